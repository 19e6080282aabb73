// processor_parse_apsara_gpu.hpp -- MI355X drop-in for LoongCollector's processor_parse_apsara_native.
//
// Mirrors core/plugin/processor/ProcessorParseApsaraNative.{h,cpp}.  What differs is where a line is read: the source values of a whole
// group make ONE device trip (lc_apsara_parse_host: apsara_parse_kernel) that returns, per line, the time (civil or epoch seconds,
// nanoseconds), the four base-field spans, the TRUE pair count and the first W pairs; lines with more pairs take ONE second trip.
// The host then applies the zone the way mktime does (lc_timestamp_zone_seconds) and Timezone, the time-failure and discard rules, and
// stitches the event with the calls the reference makes, in its order (AppendContentNoCopy: a repeated key is held twice).
//
// The per-group time cache (:92-93, :287-299, :319-320) is not modelled on the device.  It is unobservable while every matched
// date-form line's seconds format consumed exactly 19 bytes (LC_APSARA_CANON19): the same 19 bytes give the same second and "%f" starts
// at the same place.  From the first matched date-form line without that flag on, the rest of the group replays the reference's cache
// walk on the host, with the time routine of apsara_vm.hpp compiled for the host (mReplayedLines counts them).  Defined here, undefined
// in the reference: a time text shorter than the cached 19 bytes is no hit; a cache taken from a line of fewer than 20 bytes never hits.
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_apsara.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, ParseProcessorBase

namespace logtail {

class ProcessorParseApsaraGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_parse_apsara_gpu"

    // false with `error` set where the reference's Init returns false (:37-84)
    bool Init(const lcjson::Value& config, std::string& error);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    std::string mTimezone;
    int32_t mLogTimeZoneOffsetSecond = 0;
    GpuCommonParserOptions mCommonParserOptions;

    // the agent's flags the discard rule reads (:173)
    bool mDiscardOldData = true;
    int32_t mDiscardInterval = 43200;
    uint32_t mFirstTripPairs = 0;  // 0: kDefaultFirstTripPairs

    std::atomic<uint64_t> mHistoryFailureTotal{0};
    std::atomic<uint64_t> mReplayedLines{0}, mMopUpLinesTotal{0};

    void SetClock(lc_clock_t clock, void* user) {
        mClock = clock;
        mClockUser = user;
    }
    int64_t Now() const;

private:
    lc_clock_t mClock = nullptr;
    void* mClockUser = nullptr;
};

}  // namespace logtail
