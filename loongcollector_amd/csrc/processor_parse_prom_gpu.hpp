// processor_parse_prom_gpu.hpp -- MI355X drop-in for LoongCollector's processor_prom_parse_metric_native.
//
// Mirrors core/plugin/processor/inner/ProcessorPromParseMetricNative.{h,cpp} and the TextParser it drives.  What differs is where a
// line is read: the contents of a group's RawEvents make ONE device trip (lc_prom_parse_host: prom_parse_kernel, the deferred number
// tokens finished by std::strtod on the host) that returns, per line, a status, the name's span, the value, the timestamp and the
// spans of the first W labels; the lines with more labels take ONE second trip with room for the widest.  The host then builds the
// MetricEvents with the calls the reference makes, in its order: SetNameNoCopy, per label SetTagNoCopy (a view) or -- for a value that
// holds a backslash -- the copying SetTag of the text rewritten by the reference's rule, SetValue, SetTimestamp, and last the copying
// SetTag("__name__", name).
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_prom.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, ParseProcessorBase

namespace logtail {

class ProcessorParsePromGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_prom_parse_metric_gpu"

    // ScrapeConfig::InitStaticConfig's refusals that need no relabel code (lc_prom.h)
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& eGroup);

    std::string mJobName;
    bool mHonorTimestamps = true;
    std::string mConfigName;
    uint32_t mFirstTripLabels = LC_PROM_DEFAULT_LABELS;

    std::atomic<uint64_t> mDeferredTokens{0}, mMopUpLinesTotal{0};
};

}  // namespace logtail
