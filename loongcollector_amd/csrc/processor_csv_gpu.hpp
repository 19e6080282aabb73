// processor_csv_gpu.hpp -- the Go plugin processor_csv over the device decoder (include/csv/lc_csv.h).
//
// Mirrors plugins/processor/csv/processor_csv.go: the fields keep their Go names (:31-40), Init = :46-54, ProcessLogs / decodeCSV =
// :60-134 -- with the per-log csv.Reader replaced by ONE batched engine call (lc_csv_host: csv_split_kernel) over the source values of
// all logs, plus one mop-up call for the values that need more fields than the first kept.  What the engine does not know is applied
// here to its rows: the fold of a quoted field (`""`, `\r\n`), SplitKeys, ExpandOthers, the csv.Writer form of the remainder,
// KeepSource, the alarms.  Logs are the protocol.Log shape: an ordered list of (Key, Value) contents; fields are appended.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/csv/lc_csv.h"
#include "csv_vm.hpp"

namespace lccsv {

struct LogContent {
    std::string Key, Value;
};
struct Log {
    std::vector<LogContent> Contents;
};

// csv.Writer.Write + Flush for one record, without the final `\n` (fieldNeedsQuotes: non-empty and `\.`, or holds the separator, `"`,
// `\r` or `\n`, or begins with a unicode.IsSpace rune; inside the quotes `"` -> `""`)
std::string writeRecord(const std::vector<std::string>& fields, const std::string& sep);

class ProcessorCsvGpu {
public:
    // exported fields, names and defaults as in the Go (init :136-142)
    std::string SourceKey;
    bool NoKeyError = false;
    std::vector<std::string> SplitKeys;
    std::string SplitSep = ",";
    bool TrimLeadingSpace = false;
    bool PreserveOthers = false;
    bool ExpandOthers = false;
    std::string ExpandKeyPrefix;
    bool KeepSource = false;

    // Init :46-54; throws std::runtime_error("invalid separator: <SplitSep>") unless SplitSep is exactly one rune
    void Init();
    // self: the handle that holds this processor (what the engine entry takes).  LC_OK, or the engine's error code: every log is then as it was
    int ProcessLogs(const lc_csv_t* self, std::vector<Log>& logs);

    CsvConfig cfg{};
    uint32_t firstTripFields = 0;  // 0: len(SplitKeys), + LC_CSV_PRESERVE_EXTRA with PreserveOthers
    uint64_t counters[LC_CSV_CNT_COUNT] = {};
    lc_alarm_sink_t sink = nullptr;
    void* sinkUser = nullptr;

private:
    void alarm(int kind, const std::string& text) const {
        if (sink) sink(sinkUser, kind, text.data(), text.size());
    }
};

}  // namespace lccsv

struct lc_csv {
    lccsv::ProcessorCsvGpu p;
};
inline const CsvConfig& lcCsvConfig(const lc_csv* h) { return h->p.cfg; }
