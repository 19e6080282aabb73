// processor_parse_json_gpu.hpp -- MI355X drop-in for LoongCollector's processor_parse_json_native.
//
// Mirrors what the reference class configures and does
//   core/plugin/processor/ProcessorParseJsonNative.h / .cpp:44-145, :469-477
// with the policy helper CommonParserOptions (GpuCommonParserOptions of processor_parse_regex_gpu.hpp).  What differs is where the
// documents are parsed: instead of one simdjson / rapidjson parse per event (:124-128) the source values of the whole group make ONE
// device trip (lc_json_walk_host: json_walk_kernel), a second one only for lines with more top-level members than the first trip kept,
// and the member records are stitched back into the events: strings, integers, containers, true and false as zero-copy views of the
// source value, null as the empty view, escaped text copied from the trip's unescaped bytes into the group's SourceBuffer, and every
// other number through strtod and snprintf("%f") (std::to_string(double), :178) on the host.
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_json.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, GpuCommonParserOptions, ParseProcessorBase

namespace logtail {

class ProcessorParseJsonGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_parse_json_gpu"

    const std::string& Name() const { return sName; }
    // false with `error` set exactly where the reference's Init returns false (:44-61)
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    GpuCommonParserOptions mCommonParserOptions;

    // (the plugin counters of :78-81 are ParseProcessorBase's)
    std::atomic<uint64_t> mMopUpLinesTotal{0};   // no reference counterpart: lines that took the second trip
    std::atomic<uint64_t> mShadowBytesTotal{0};  // no reference counterpart: unescaped bytes that came back from the device
    // W of the first trip; 0 = 32, the reference's tempFields.reserve(32) (:309).  Not a config key:
    // lc_json_processor_set_first_trip_members (results do not depend on it, only how many lines take the second trip)
    uint32_t mFirstTripMembers = 0;

    // alarms (SetAlarmSink): kind 0 "parse json fail:<line>" (:278-283), kind 3: a failed device trip

private:
    // :122-144 for one event whose line the device has walked; false: the event is erased
    bool FinishEvent(LogEvent& ev, StringView raw, uint8_t status, uint32_t nmembers, const lc_json_member_t* members, const uint8_t* shadow,
                     const GroupMetadata& metadata, Tally& tally);
};

}  // namespace logtail
