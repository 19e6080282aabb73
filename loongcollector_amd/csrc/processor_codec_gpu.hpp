// processor_codec_gpu.hpp -- the Go plugins processor_base64_encoding, processor_base64_decoding and processor_md5 over the device
// codecs (include/codec/lc_codec.h).
//
// Mirrors plugins/processor/base64/encoding/processor_base64_encoding.go, plugins/processor/base64/decoding/processor_base64_decoding.go
// and plugins/processor/md5/processor_md5.go: the fields keep their Go names, ProcessLogs is the shell the three share -- with the
// per-content EncodeToString / DecodeString / md5.Sum replaced by ONE batched engine call (lc_codec_apply_host) over the first content of
// every log whose key is SourceKey.  What the engine does not know is applied here to its flags and bytes: NewKey / MD5Key, the alarms,
// the counters.  Logs are the protocol.Log shape: an ordered list of (Key, Value) contents.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/codec/lc_codec.h"
#include "codec_vm.hpp"

namespace lccodec {

struct LogContent {
    std::string Key, Value;
};
struct Log {
    std::vector<LogContent> Contents;
};

class ProcessorCodecGpu {
public:
    // exported fields, names as in the Go; Op is this project's selector
    std::string Op, SourceKey, NewKey, MD5Key;
    bool NoKeyError = false, DecodeError = false;

    // LC_OK, or LC_ERR_ARG with *why set: a missing or unknown Op.  (The reference's Init refuses nothing.)
    int Init(std::string* why);
    // self: the handle that holds this processor (what the engine entry takes).  LC_OK, or the engine's error code: every log is then as it was
    int ProcessLogs(const lc_codec_t* self, std::vector<Log>& logs);

    CodecConfig cfg{};
    uint64_t counters[LC_CODEC_CNT_COUNT] = {};
    lc_alarm_sink_t sink = nullptr;
    void* sinkUser = nullptr;

private:
    void alarm(int kind, const std::string& text) const {
        if (sink) sink(sinkUser, kind, text.data(), text.size());
    }
};

}  // namespace lccodec

struct lc_codec {
    lccodec::ProcessorCodecGpu p;
};
inline const CodecConfig& lcCodecConfig(const lc_codec* h) { return h->p.cfg; }
