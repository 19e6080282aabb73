// processor_parse_timestamp_gpu.hpp -- MI355X drop-in for LoongCollector's processor_parse_timestamp_native.
//
// Mirrors core/plugin/processor/ProcessorParseTimestampNative.{h,cpp} with Strptime() / DeduceYear / ParseLogTimeZoneOffsetSecond of
// core/common/TimeUtil.cpp.  What differs is where the format is interpreted: the time fields of a whole group make ONE device trip
// (lc_strptime_parse_host: strptime_kernel) that returns, per value, civil seconds, nanoseconds, the matched length and same_as_prev.
// The host then
//   * applies the process's local zone the way mktime does (a per-day cache of the UTC offset; a day that holds a transition goes
//     through mktime itself), the year modes and SourceTimezone;
//   * reproduces the reference's per-group string cache (ParseLogTime :181-241) -- observable: a value that has the cached string as
//     a prefix takes the cached second -- by walking only run heads and values whose same_as_prev bit is clear.  Inside a run of set
//     bits the cache holds exactly the run's matched prefix, so every value of the run hits it and takes the second the run's head
//     left behind.
// processor_parse_apsara_native is processor_parse_apsara_gpu.hpp.  Out of scope: the precise-timestamp key the reference has commented out (:172-176, :233-239).
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lc_timestamp.h"
#include "parse_processor_shell.hpp"  // the event model, json_min, ParseProcessorBase

namespace logtail {

class ProcessorParseTimestampGpu : public ParseProcessorBase {
public:
    static const std::string sName;  // "processor_parse_timestamp_gpu"
    ~ProcessorParseTimestampGpu();

    // false with `error` set where the reference's Init returns false (:30-98); *unsupported: the format exceeds the program window
    bool Init(const lcjson::Value& config, std::string& error, bool* unsupported = nullptr);
    // LC_OK, or the LC_ERR_* code of a failed device trip (the group is then untouched)
    int Process(PipelineEventGroup& logGroup);

    std::string mSourceFormat;
    std::string mSourceTimezone;
    int32_t mSourceYear = -1;
    int32_t mLogTimeZoneOffsetSecond = 0;

    // the agent's flags and pipeline property the discard rule reads (:146-149)
    bool mDiscardOldData = true;
    int32_t mDiscardInterval = 43200;
    bool mOnetime = false;
    bool mPlainWalk = false;  // walk every value (the tests compare it with the run-head walk)

    std::atomic<uint64_t> mHistoryFailureTotal{0};  // (beside ParseProcessorBase's counters: every discarded event counts here too)
    std::atomic<uint64_t> mWalkedValues{0}, mRunValues{0};

    void SetClock(lc_clock_t clock, void* user) {
        mClock = clock;
        mClockUser = user;
    }
    int64_t Now() const;

private:
    // tv_sec as Strptime() leaves it for one device result (mktime, the year modes); no SourceTimezone yet
    int64_t LocalSeconds(uint8_t status, int64_t secs, int64_t now) const;

    lc_clock_t mClock = nullptr;
    void* mClockUser = nullptr;
    bool mHaveNanosecond = false, mEndWithNanosecond = false, mFormatIsEpoch = false, mFormatIsFraction = false;
    lc_strptime_t* mStrptime = nullptr;
};

}  // namespace logtail
