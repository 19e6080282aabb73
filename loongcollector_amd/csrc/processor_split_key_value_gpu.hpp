// processor_split_key_value_gpu.hpp -- the Go plugin processor_split_key_value over the device splitter (include/kvsplit/lc_kvsplit.h).
//
// Mirrors plugins/processor/split/keyvalue/key_value_splitter.go: the fields keep their Go names (:27-44), Init = :53-69 over the
// defaults of newKeyValueSplitter :194-206, ProcessLogs / processLog = :75-97 -- with the per-log splitKeyValue replaced by ONE batched
// engine call (lc_kvsplit_host: kv_split_kernel) over the source values of all logs, plus one mop-up call for the values with more
// pairs than the first kept.  What the engine does not know is applied here to its rows: DiscardWhenSeparatorNotFound, the two key
// prefixes with their running indices, the three ErrIf* alarms.  Logs are the protocol.Log shape: an ordered list of (Key, Value)
// contents; pairs are appended, duplicates kept.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/kvsplit/lc_kvsplit.h"
#include "kv_vm.hpp"

namespace lckv {

struct LogContent {
    std::string Key, Value;
};
struct Log {
    std::vector<LogContent> Contents;
};

class ProcessorSplitKeyValueGpu {
public:
    // exported fields, names and defaults as in the Go (newKeyValueSplitter)
    std::string SourceKey;
    std::string Delimiter = "\t";
    std::string Separator = ":";
    bool KeepSource = true;
    std::string EmptyKeyPrefix = "empty_key_";
    std::string NoSeparatorKeyPrefix = "no_separator_key_";
    std::string Quote;
    bool DiscardWhenSeparatorNotFound = false;
    bool ErrIfSourceKeyNotFound = true;
    bool ErrIfSeparatorNotFound = true;
    bool ErrIfKeyIsEmpty = true;

    // Init :53-69; throws std::runtime_error for a needle above LC_KV_MAX_NEEDLE bytes
    void Init();
    // self: the handle that holds this processor (what the engine entry takes).  LC_OK, or the engine's error code: every log is then as it was
    int ProcessLogs(const lc_kvsplit_t* self, std::vector<Log>& logs);

    KvConfig cfg{};
    uint32_t firstTripPairs = LC_KV_DEFAULT_PAIRS;
    uint64_t counters[LC_KV_CNT_COUNT] = {};
    lc_alarm_sink_t sink = nullptr;
    void* sinkUser = nullptr;

private:
    void alarm(int kind, const std::string& text) const {
        if (sink) sink(sinkUser, kind, text.data(), text.size());
    }
};

}  // namespace lckv

struct lc_kvsplit {
    lckv::ProcessorSplitKeyValueGpu p;
};
inline const KvConfig& lcKvConfig(const lc_kvsplit* h) { return h->p.cfg; }
