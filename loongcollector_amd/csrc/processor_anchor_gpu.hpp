// processor_anchor_gpu.hpp -- the Go plugin processor_anchor over the device locator (include/anchor/lc_anchor.h).
//
// Mirrors plugins/processor/anchor/anchor.go: the fields keep their Go names (:46-68, the reference's spellings ExpondJSON /
// ExpondConnecter included), Init = :74-99, ProcessLogs / ProcessLog = :105-129 -- with the per-log ProcessAnchor replaced by ONE
// batched engine call (lc_anchor_locate_host: anchor_locate_kernel) over the source values of all logs that have the key.  What the
// engine does not know is applied here to its rows: KeepSource, the field names, the three alarms, the pairs-per-log metric.  Logs are
// the protocol.Log shape: an ordered list of (Key, Value) contents; fields are appended, duplicates kept.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/anchor/lc_anchor.h"
#include "anchor_vm.hpp"

namespace lcanchor {

struct LogContent {
    std::string Key, Value;
};
struct Log {
    std::vector<LogContent> Contents;
};

struct Anchor {
    std::string Start, Stop, FieldName, FieldType;
    // accepted and meaningless for the string type (DEFINED in lc_anchor.h: a json anchor is refused)
    bool ExpondJSON = false, IgnoreJSONError = false;
    std::string ExpondConnecter;
    int64_t MaxExpondDepth = 0;
};

class ProcessorAnchorGpu {
public:
    // exported fields, names as in the Go; no defaults
    std::vector<Anchor> Anchors;
    bool NoKeyError = false;
    bool NoAnchorError = false;
    std::string SourceKey;
    bool KeepSource = false;

    // Init :74-99; throws std::runtime_error for a json anchor, a seventeenth anchor, a needle above LC_ANCHOR_MAX_NEEDLE bytes
    void Init();
    // self: the handle that holds this processor (what the engine entry takes).  LC_OK, or the engine's error code: every log is then as it was
    int ProcessLogs(const lc_anchor_t* self, std::vector<Log>& logs);

    AnchorConfig cfg{};
    uint64_t counters[LC_ANCHOR_CNT_COUNT] = {};
    lc_alarm_sink_t sink = nullptr;
    void* sinkUser = nullptr;

private:
    void alarm(int kind, const std::string& text) const {
        if (sink) sink(sinkUser, kind, text.data(), text.size());
    }
};

}  // namespace lcanchor

struct lc_anchor {
    lcanchor::ProcessorAnchorGpu p;
};
inline const AnchorConfig& lcAnchorConfig(const lc_anchor* h) { return h->p.cfg; }
