// processor_string_replace_gpu.hpp -- the Go plugin processor_string_replace, methods const and unquote, over the device rewrite
// (include/strrep/lc_strrep.h).
//
// Mirrors plugins/processor/stringreplace/processor_string_replace.go: the fields keep their Go names (:41-54), Init = :61-95,
// ProcessLogs = :101-140 -- with the per-content strings.ReplaceAll / strconv.Unquote replaced by ONE batched engine call
// (lc_strrep_apply_host: strrep_size_kernel, the scan, strrep_write_kernel) over every content of the batch whose key is SourceKey.
// What the engine does not know is applied here to its flags and bytes: DestKey, the alarm, the metric.  Logs are the protocol.Log
// shape: an ordered list of (Key, Value) contents.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/strrep/lc_strrep.h"
#include "strrep_vm.hpp"

namespace lcstrrep {

struct LogContent {
    std::string Key, Value;
};
struct Log {
    std::vector<LogContent> Contents;
};

class ProcessorStringReplaceGpu {
public:
    // exported fields, names as in the Go
    std::string SourceKey, Method, Match, ReplaceString, DestKey;
    int64_t RegexTimeoutMs = 0;  // accepted and ignored: there is no regex here

    // Init :61-95 and the bounds lc_strrep.h defines.  LC_OK, or the code with *why set.
    int Init(std::string* why);
    // self: the handle that holds this processor (what the engine entry takes).  LC_OK, or the engine's error code: every log is then as it was
    int ProcessLogs(const lc_strrep_t* self, std::vector<Log>& logs);

    StrrepConfig cfg{};
    uint64_t counters[LC_STRREP_CNT_COUNT] = {};
    lc_alarm_sink_t sink = nullptr;
    void* sinkUser = nullptr;

private:
    void alarm(int kind, const std::string& text) const {
        if (sink) sink(sinkUser, kind, text.data(), text.size());
    }
};

}  // namespace lcstrrep

struct lc_strrep {
    lcstrrep::ProcessorStringReplaceGpu p;
};
inline const StrrepConfig& lcStrrepConfig(const lc_strrep* h) { return h->p.cfg; }
