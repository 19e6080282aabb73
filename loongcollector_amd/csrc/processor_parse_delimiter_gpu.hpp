// processor_parse_delimiter_gpu.hpp -- MI355X drop-in for LoongCollector's processor_parse_delimiter_native.
//
// Mirrors, member for member, what the reference class configures
//   core/plugin/processor/ProcessorParseDelimiterNative.h / .cpp:30-419
// with its parser core/parser/DelimiterModeFsmParser.cpp and the policy helper CommonParserOptions (GpuCommonParserOptions of
// processor_parse_regex_gpu.hpp).  What differs is where the lines are split: instead of one ParseDelimiterLine / SplitString call per
// event (:253-282) the source values of the whole group make ONE device trip (lc_delim_split_host: delim_split_kernel), a second one
// only for lines with more columns than the first trip kept, and the (begin, end) table is stitched back into the events as zero-copy
// views (:325-348), doubled quotes folded into the group's SourceBuffer exactly as AddFieldWithUnQuote does.
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_delimiter.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, GpuCommonParserOptions, ParseProcessorBase

namespace logtail {

class ProcessorParseDelimiterGpu : public ParseProcessorBase {
public:
    static const std::string sName;                 // "processor_parse_delimiter_gpu"
    static const std::string s_mDiscardedFieldKey;  // "_"
    enum class OverflowedFieldsTreatment { EXTEND, KEEP, DISCARD };
    ~ProcessorParseDelimiterGpu();

    const std::string& Name() const { return sName; }
    // false with `error` set exactly where the reference's Init returns false (:30-184)
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    std::string mSeparator;
    char mSeparatorChar = '\0';
    char mQuote = '"';
    std::vector<std::string> mKeys;
    bool mAllowingShortenedFields = false;
    OverflowedFieldsTreatment mOverflowedFieldsTreatment = OverflowedFieldsTreatment::EXTEND;
    bool mExtractingPartialFields = false;
    GpuCommonParserOptions mCommonParserOptions;

    // (the plugin counters of :178-181 are ParseProcessorBase's)
    std::atomic<uint64_t> mMopUpLinesTotal{0};  // no reference counterpart: lines that took the second trip
    // W of the first trip; 0 = the reference's reserve (:244-245).  Not a config key: lc_delimiter_processor_set_first_trip_columns
    // (set before the first Process; results do not depend on it, only how many lines take the second trip)
    uint32_t mFirstTripColumns = 0;

    // alarms (SetAlarmSink): kind 0 "parse delimiter log fail, logs:<line>" (:303-309), kind 2 "keys count unmatch columns count :<n>,
    // required:<k>, logs:<line>" (:292-299), kind 4 "no column keys defined" (:313-318), kind 3: a failed device trip

private:
    // one column's value: a view of the line, or its un-doubled copy in the group's SourceBuffer (AddFieldWithUnQuote :83-113)
    StringView ColumnValue(LogEvent& ev, StringView raw, int32_t begin, int32_t end) const;
    // :284-363 for one event whose line the device has split; false: the event is erased
    bool FinishEvent(LogEvent& ev, StringView raw, uint8_t status, uint32_t ncols, const int32_t* spans, const GroupMetadata& metadata,
                     Tally& tally);

    bool mSourceKeyOverwritten = false;
    bool mUseQuote = false;
    lc_delim_t* mDelim = nullptr;
};

}  // namespace logtail
