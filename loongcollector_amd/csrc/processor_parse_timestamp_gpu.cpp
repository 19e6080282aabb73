// processor_parse_timestamp_gpu.cpp -- see processor_parse_timestamp_gpu.hpp.
#include "processor_parse_timestamp_gpu.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "strptime_vm.hpp"

// ---------------------------------------------------------------------------------------------- the local zone
// mktime(fields) = civil seconds - (the zone's UTC offset at that local time).  The offset is constant over a civil day unless the day
// holds a transition, so it is cached per (day, tm_isdst); a day whose ends disagree -- under the caller's tm_isdst or under -1 -- is
// marked and every value on it goes through mktime.  The cache belongs to the thread: no lock, and glibc's own lock is only met on a miss.
namespace {
struct ZoneDay {
    int64_t key = INT64_MIN;  // day * 2 + dst
    int64_t offset = 0;
    bool viaMktime = false;
};
constexpr size_t kZoneSlots = 64;
struct ZoneCache {
    ZoneDay slot[kZoneSlots];
    uint64_t generation = 0;
};
thread_local ZoneCache tlsZone;
std::atomic<uint64_t> gZoneGeneration{1};

void civilToTm(int64_t civil, int dst, struct tm* tm) {
    int64_t days = civil / 86400, rem = civil % 86400;
    if (rem < 0) {
        rem += 86400;
        --days;
    }
    // civil-from-days (proleptic Gregorian)
    int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    const int64_t d = doy - (153 * mp + 2) / 5 + 1;
    const int64_t m = mp < 10 ? mp + 3 : mp - 9;
    const int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
    std::memset(tm, 0, sizeof *tm);
    tm->tm_year = int(y - 1900);
    tm->tm_mon = int(m - 1);
    tm->tm_mday = int(d);
    tm->tm_hour = int(rem / 3600);
    tm->tm_min = int(rem % 3600 / 60);
    tm->tm_sec = int(rem % 60);
    tm->tm_isdst = dst;
}
int64_t mktimeOfCivil(int64_t civil, int dst) {
    struct tm tm;
    civilToTm(civil, dst, &tm);
    return int64_t(mktime(&tm));
}
}  // namespace

extern "C" int64_t lc_timestamp_zone_seconds(int64_t civil, int dst) {
    dst = dst ? 1 : 0;
    ZoneCache& Z = tlsZone;
    const uint64_t gen = gZoneGeneration.load(std::memory_order_relaxed);
    if (Z.generation != gen) {
        for (ZoneDay& s : Z.slot) s.key = INT64_MIN;
        Z.generation = gen;
    }
    int64_t day = civil / 86400;
    if (civil % 86400 < 0) --day;
    const int64_t key = day * 2 + dst;
    ZoneDay& s = Z.slot[size_t(uint64_t(key) % kZoneSlots)];
    if (s.key != key) {
        const int64_t a = day * 86400, b = a + 86400;
        const int64_t offA = a - mktimeOfCivil(a, dst), offB = b - mktimeOfCivil(b, dst);
        const int64_t autoA = a - mktimeOfCivil(a, -1), autoB = b - mktimeOfCivil(b, -1);
        s.key = key;
        s.offset = offA;
        s.viaMktime = offA != offB || autoA != autoB;
    }
    return s.viaMktime ? mktimeOfCivil(civil, dst) : civil - s.offset;
}
extern "C" void lc_timestamp_zone_reset(void) { gZoneGeneration.fetch_add(1); }

namespace logtail {

const std::string ProcessorParseTimestampGpu::sName = "processor_parse_timestamp_gpu";

namespace {
struct ProcessScratch {
    std::vector<uint8_t> kind, status, same;
    std::vector<const uint8_t*> ptr;
    std::vector<uint32_t> len, nanos;
    std::vector<int64_t> secs;
    std::vector<int32_t> matched, fracLen;
};
}  // namespace

ProcessorParseTimestampGpu::~ProcessorParseTimestampGpu() {
    if (mStrptime) lc_strptime_destroy(mStrptime);
}

int64_t ProcessorParseTimestampGpu::Now() const { return mClock ? mClock(mClockUser) : int64_t(time(nullptr)); }

// ProcessorParseTimestampNative::Init :30-98
bool ProcessorParseTimestampGpu::Init(const lcjson::Value& config, std::string& error, bool* unsupported) {
    if (unsupported) *unsupported = false;
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    if (!mandatoryString(config, "SourceKey", mSourceKey, error)) return false;
    if (!mandatoryString(config, "SourceFormat", mSourceFormat, error)) return false;
    // SourceTimezone :58-76
    {
        const lcjson::Value* v = config.find("SourceTimezone");
        if (v && !v->isString()) {
            mInitWarnings.push_back("param SourceTimezone is not of type string");
        } else {
            if (v) mSourceTimezone = v->str;
            // ParseLogTimeZoneOffsetSecond (TimeUtil.cpp:428-438)
            if (!mSourceTimezone.empty()) {
                int tzSecond = 0;
                if (!parseTimeZoneOffsetSecond(mSourceTimezone, tzSecond)) {
                    mInitWarnings.push_back("string param SourceTimezone is not valid");
                } else {
                    const time_t nowTime = time_t(Now());
                    struct tm info;
                    std::memset(&info, 0, sizeof info);
                    localtime_r(&nowTime, &info);
                    mLogTimeZoneOffsetSecond = tzSecond - int32_t(info.tm_gmtoff);
                }
            }
        }
    }
    // SourceYear :79-89
    if (const lcjson::Value* v = config.find("SourceYear")) {
        if (!v->isNumber() || v->num != double(int64_t(v->num)) || v->num < double(INT32_MIN) || v->num > double(INT32_MAX))
            mInitWarnings.push_back("param SourceYear is not of type int");
        else
            mSourceYear = int32_t(v->num);
    }
    // ParseLogTime's view of the format (:190-192)
    const char* f = std::strstr(mSourceFormat.c_str(), "%f");
    mHaveNanosecond = f != nullptr;
    mEndWithNanosecond = f == mSourceFormat.c_str() + mSourceFormat.size() - 2;
    mFormatIsEpoch = mSourceFormat == "%s";
    mFormatIsFraction = std::strcmp(mSourceFormat.c_str(), "%f") == 0;
    char err[256];
    const int rc = lc_strptime_create(mSourceFormat.c_str(), &mStrptime, err, sizeof err);
    if (rc != LC_OK) {
        error = std::string("SourceFormat cannot run on the device: ") + err;
        if (unsupported) *unsupported = true;
        return false;
    }
    return true;
}

// Strptime() behind strptime_ns (TimeUtil.cpp:141-190)
int64_t ProcessorParseTimestampGpu::LocalSeconds(uint8_t status, int64_t secs, int64_t now) const {
    if (status & LC_TS_EPOCH) return secs;  // mktime(localtime(t)) = t
    const int dst = (status & LC_TS_DST) ? 1 : 0;
    if (status & LC_TS_HAS_YEAR) return lc_timestamp_zone_seconds(secs, dst);
    const int mon = int((secs >> 40) & 0xff), mday = int((secs >> 32) & 0xff);
    const int64_t tod = secs & 0xffffffff;
    int64_t year;
    if (mSourceYear < 0) {
        // the fields go to mktime with tm_year = INT_MIN, as the reference leaves them: libc decides (glibc answers with a large
        // negative second, see the floor vectors without a year; the event is dropped by the tv_sec <= 0 rule)
        struct tm tm;
        std::memset(&tm, 0, sizeof tm);
        tm.tm_year = INT_MIN;
        tm.tm_mon = mon;
        tm.tm_mday = mday;
        tm.tm_hour = int(tod / 3600);
        tm.tm_min = int(tod % 3600 / 60);
        tm.tm_sec = int(tod % 60);
        tm.tm_isdst = dst;
        return int64_t(mktime(&tm));
    } else if (mSourceYear > 0) {
        year = mSourceYear;
    } else {
        // DeduceYear (:123-135) against the clock's local date
        const time_t t = time_t(now);
        struct tm cur;
        std::memset(&cur, 0, sizeof cur);
        if (!localtime_r(&t, &cur)) {
            // (the reference returns here and leaves tv_sec as it was; a clock libc cannot break down does not occur on a 64-bit
            // time_t within +-2^55 s, and the conversion with tm_year = 0 that follows is this port's own choice for that case)
            year = 1900;
        } else if (mon == 0 && mday == 1 && cur.tm_mon == 11 && cur.tm_mday == 31) {
            year = int64_t(cur.tm_year) + 1 + 1900;
        } else if (mon == 11 && mday == 31 && cur.tm_mon == 0 && cur.tm_mday == 1) {
            year = int64_t(cur.tm_year) - 1 + 1900;
        } else {
            year = int64_t(cur.tm_year) + 1900;
        }
    }
    return lc_timestamp_zone_seconds(tsCivilSeconds(year, uint32_t(mon), mday, tod), dst);
}

// Process :100-120 + ProcessEvent :126-179 + ParseLogTime :181-241, restructured as gather -> device trip -> walk
int ProcessorParseTimestampGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty() || mSourceFormat.empty() || mSourceKey.empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    gatherSourceValues(events, mSourceKey, S.kind, S.ptr, S.len);  // (the walk below counts the events without a value as it meets them)
    const uint32_t nValues = uint32_t(S.ptr.size());
    if (nValues) {
        S.status.resize(nValues);
        S.same.resize(nValues);
        S.secs.resize(nValues);
        S.nanos.resize(nValues);
        S.matched.resize(nValues);
        S.fracLen.resize(nValues);
        const lc_ts_out_t out{S.status.data(), S.secs.data(), S.nanos.data(), S.matched.data(), S.fracLen.data(), S.same.data()};
        const int rc = lc_strptime_parse_host(mStrptime, S.ptr.data(), S.len.data(), nValues, &out);
        if (rc != LC_OK) return ReportFailedTrip(sName, "timestamp parse", "without a parsed time", rc, nValues);
    }
    const int64_t now = Now();
    const bool cacheInUse = !mHaveNanosecond || mEndWithNanosecond;
    // the walk's state: ParseLogTime's timeStrCache and the LogtailTime that lives across the group's events (:105-107)
    const uint8_t* cache = nullptr;
    uint32_t cacheLen = 0;
    int64_t tvSec = 0;
    bool cacheIsPrevPrefix = false;  // the cache holds exactly the matched prefix of the value before, which parsed
    Tally tally;
    uint64_t walked = 0, inRun = 0;
    size_t vi = 0;
    compactEvents(events, [&](size_t rIdx) {
        bool keep = true;
        if (S.kind[rIdx] == kNotLogEvent) {
            ++tally.outFailed;
        } else if (S.kind[rIdx] == kNoSourceKey) {
            ++tally.keyNotFound;
        } else {
            const size_t i = vi++;
            const uint8_t* val = S.ptr[i];
            const uint32_t len = S.len[i];
            const bool ok = S.status[i] & LC_TS_OK;
            const uint32_t prefix = uint32_t(S.matched[i] - S.fracLen[i]);
            bool parsed = false;
            uint32_t nsec = 0;
            if (cacheInUse && !mPlainWalk && S.same[i] && cacheIsPrevPrefix) {
                // inside a run: the cache is this value's own matched prefix, so the value hits it (:195-202) and keeps tvSec
                ++inRun;
                if (mEndWithNanosecond || (mFormatIsEpoch && len > cacheLen)) {
                    parsed = S.fracLen[i] > 0;  // Strptime(value + cache, "%f"): the digits the device read at that very place
                    nsec = S.nanos[i];
                } else {
                    parsed = true;
                }
            } else {
                ++walked;
                const bool hit = cacheInUse && cacheLen > 0 && len >= cacheLen && std::memcmp(val, cache, cacheLen) == 0;  // IsPrefixString
                if (hit) {
                    if (mEndWithNanosecond || (mFormatIsEpoch && len > cacheLen)) {
                        uint32_t pos = cacheLen;
                        int32_t digits = 0;
                        parsed = tsConvNanos(HostSpanSource{val}, len, pos, nsec, digits);
                    } else {
                        parsed = true;
                    }
                } else {
                    // Strptime() sets tv_sec whether or not the format matched (a format that is "%f" alone returns before it does)
                    if (!mFormatIsFraction) tvSec = LocalSeconds(S.status[i], S.secs[i], now);
                    if (ok) {
                        parsed = true;
                        nsec = S.nanos[i];
                        cache = val;
                        cacheLen = prefix;  // :208-212
                        tvSec -= mLogTimeZoneOffsetSecond;
                    }
                }
                cacheIsPrevPrefix = ok && cacheLen == prefix && (hit || parsed);
            }
            if (!parsed) {
                RaiseAlarm(0, std::string(reinterpret_cast<const char*>(val), len) + " " + mSourceFormat);  // :223-228
                ++tally.outFailed;
            } else if (tvSec <= 0 || (mDiscardOldData && (now - tvSec) > mDiscardInterval && !mOnetime)) {  // :146-170
                RaiseAlarm(1, "logTime: " + std::to_string(tvSec));
                ++tally.discarded;
                keep = false;
            } else {
                events[rIdx].Cast<LogEvent>().SetTimestamp(time_t(tvSec), nsec);
                ++tally.outSuccessful;
            }
        }
        return keep;
    });
    AddTally(tally);
    if (tally.discarded) mHistoryFailureTotal += tally.discarded;
    mWalkedValues += walked;
    mRunValues += inRun;
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_timestamp.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseTimestampGpu;

struct lc_timestamp_processor : logtail::ProcessorHandle<ProcessorParseTimestampGpu> {};

extern "C" int lc_timestamp_processor_create(const char* config_json, lc_timestamp_processor_t** out, char* err, size_t errcap) {
    return lc_timestamp_processor_create_with_clock(config_json, nullptr, nullptr, out, err, errcap);
}
extern "C" int lc_timestamp_processor_create_with_clock(const char* config_json, lc_clock_t clock, void* clock_user,
                                                        lc_timestamp_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap, [&](lc_timestamp_processor& h, const lcjson::Value& cfg, std::string& error) {
        h.impl.SetClock(clock, clock_user);  // Init resolves SourceTimezone against it
        bool unsupported = false;
        if (h.impl.Init(cfg, error, &unsupported)) return int(LC_OK);
        return int(unsupported ? LC_ERR_UNSUPPORTED : LC_ERR_SYNTAX);
    });
}
extern "C" void lc_timestamp_processor_destroy(lc_timestamp_processor_t* p) { delete p; }
extern "C" char* lc_timestamp_processor_warnings(const lc_timestamp_processor_t* p) { return logtail::warningsText(p); }
extern "C" int32_t lc_timestamp_processor_zone_offset(const lc_timestamp_processor_t* p) { return p ? p->impl.mLogTimeZoneOffsetSecond : 0; }
extern "C" int lc_timestamp_processor_process_native(lc_timestamp_processor_t* p, void* native_group) {
    return logtail::processNative(p, native_group);
}
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_timestamp_processor_process(lc_timestamp_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" void lc_timestamp_processor_set_clock(lc_timestamp_processor_t* p, lc_clock_t clock, void* user) {
    if (p) p->impl.SetClock(clock, user);
}
extern "C" void lc_timestamp_processor_set_discard(lc_timestamp_processor_t* p, int discard_old_data, int32_t interval_seconds, int onetime) {
    if (!p) return;
    p->impl.mDiscardOldData = discard_old_data != 0;
    p->impl.mDiscardInterval = interval_seconds;
    p->impl.mOnetime = onetime != 0;
}
extern "C" void lc_timestamp_processor_set_plain_walk(lc_timestamp_processor_t* p, int on) {
    if (p) p->impl.mPlainWalk = on != 0;
}
extern "C" void lc_timestamp_processor_walk_stats(const lc_timestamp_processor_t* p, uint64_t out[2]) {
    if (!p || !out) return;
    out[0] = p->impl.mWalkedValues;
    out[1] = p->impl.mRunValues;
}
extern "C" int lc_timestamp_processor_counters(const lc_timestamp_processor_t* p, uint64_t out[LC_CNT_COUNT]) {
    return logtail::fillCounters(p, out, true);
}
extern "C" uint64_t lc_timestamp_processor_history_failures(const lc_timestamp_processor_t* p) { return p ? uint64_t(p->impl.mHistoryFailureTotal) : 0; }
extern "C" void lc_timestamp_processor_set_alarm_sink(lc_timestamp_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_parse_timestamp_gpu)
extern "C" int lcTimestampSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_timestamp_processor_create, ProcessorParseTimestampGpu::sName, config_text, state);
}
extern "C" void lcTimestampSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_timestamp_processor_t*>(state), native_group);
}
extern "C" void lcTimestampSlotFinalize(void* state) { delete static_cast<lc_timestamp_processor_t*>(state); }
