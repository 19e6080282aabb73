// processor_desensitize_gpu.hpp -- MI355X drop-in for LoongCollector's processor_desensitize_native.
//
// Mirrors core/plugin/processor/ProcessorDesensitizeNative.{h,cpp}.  What differs is where a value is searched and rewritten: the
// SourceKey values of a whole group make ONE device trip (lc_desens_apply_host: the match kernels in rounds, desens_collect_kernel,
// desens_size_kernel, desens_write_kernel) that returns, per value, whether it changed and where its new bytes lie.  The new bytes of
// the group are copied ONCE into the group's SourceBuffer and every changed event gets SetContentNoCopy(SourceKey, view); an unchanged
// value keeps its view.  (The reference copies every value, changed or not: no reader of the group can tell.)
//
// Failure policy (include/lc_desensitize.h): a failed trip leaves the group untouched, is alarmed (kind 3), counted and RETURNED; a value
// whose search gave up stays unchanged, is counted under LC_CNT_COMPLEXITY_EXCEEDED and alarmed (kind 1) with its event index.
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_desensitize.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, ParseProcessorBase

namespace logtail {

class ProcessorDesensitizeGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_desensitize_gpu"
    ~ProcessorDesensitizeGpu() { lc_desens_free(mEngine); }

    // false with the reference's message where its Init fails (:28-144); a ReplacingAll of the wrong type is a warning
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    int mMethod = LC_DESENS_CONST;
    std::string mReplacingString, mContentPatternBeforeReplacedString, mReplacedContentPattern;
    bool mReplacingAll = false;
    lc_desens_t* mEngine = nullptr;

    std::atomic<uint64_t> mComplexityExceededEventsTotal{0}, mRoundsTotal{0};
};

}  // namespace logtail
