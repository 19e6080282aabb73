// processor_parse_apsara_gpu.cpp -- see processor_parse_apsara_gpu.hpp.
#include "processor_parse_apsara_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "apsara_vm.hpp"

namespace logtail {

const std::string ProcessorParseApsaraGpu::sName = "processor_parse_apsara_gpu";

namespace {
const std::string SLS_KEY_LEVEL = "__LEVEL__", SLS_KEY_THREAD = "__THREAD__", SLS_KEY_FILE = "__FILE__", SLS_KEY_LINE = "__LINE__";
const std::string kMicrotimeKey = "microtime";
constexpr uint32_t kDefaultFirstTripPairs = 16;
constexpr uint32_t kCachedTimeBytes = 19;  // :318-319

// one runner thread's scratch for Process()
struct Results {
    std::vector<uint8_t> status;
    std::vector<int64_t> secs;
    std::vector<uint32_t> nanos, npairs;
    std::vector<int32_t> base, pairs;
    lc_apsara_out_t resize(uint32_t n, uint32_t W) {
        status.resize(n);
        secs.resize(n);
        nanos.resize(n);
        npairs.resize(n);
        base.resize(size_t(n) * 8);
        pairs.resize(size_t(n) * W * 3);
        return lc_apsara_out_t{status.data(), secs.data(), nanos.data(), base.data(), npairs.data(), pairs.data()};
    }
};
struct ProcessScratch {
    std::vector<uint8_t> kind, wanted;
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen;
    Results first, second;
    SecondTrip mopUp;
};

// LogEvent::AppendContentNoCopy (LogEvent.cpp:159-163): no look-up, a key that is present already is held twice.  The stand-in event
// model spells it as its bulk append of one
inline void appendContent(LogEvent& ev, StringView key, StringView val) {
#ifdef LC_USE_REFERENCE_HEADERS
    ev.AppendContentNoCopy(key, val);
#else
    ev.AppendContentsNoCopy(&key, &val, 1);
#endif
}

// the bytes the reference hands to Strptime in the replay: behind '[', up to and with the first ']' (:279-285); 0: there is none
uint32_t timeTextLength(const uint8_t* line, uint32_t len) {
    if (len < 2) return 0;
    const void* at = std::memchr(line + 1, ']', len - 1);
    return at ? uint32_t(static_cast<const uint8_t*>(at) - line) : 0u;
}
}  // namespace

int64_t ProcessorParseApsaraGpu::Now() const { return mClock ? mClock(mClockUser) : int64_t(time(nullptr)); }

// ProcessorParseApsaraNative::Init :37-84
bool ProcessorParseApsaraGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    if (!mandatoryString(config, "SourceKey", mSourceKey, error)) return false;  // :41-50
    std::string err;
    if (!optionalString(config, "Timezone", mTimezone, err)) {  // :53-71
        mInitWarnings.push_back(err);
    } else if (!mTimezone.empty()) {  // ParseLogTimeZoneOffsetSecond (TimeUtil.cpp:428-438)
        int tzSecond = 0;
        if (!parseTimeZoneOffsetSecond(mTimezone, tzSecond)) {
            mInitWarnings.push_back("string param Timezone is not valid");
        } else {
            const time_t nowTime = time_t(Now());
            struct tm info;
            std::memset(&info, 0, sizeof info);
            localtime_r(&nowTime, &info);
            mLogTimeZoneOffsetSecond = tzSecond - int32_t(info.tm_gmtoff);
        }
    }
    return mCommonParserOptions.Init(config, mInitWarnings);  // :73-75
}

// Process :86-106 + ProcessEvent :116-241, restructured as gather -> device trip(s) -> stitch
int ProcessorParseApsaraGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    const GroupMetadata& metadata = logGroup.GetAllMetadata();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    SecondTrip& T = S.mopUp;
    Tally tally;
    const Gathered gathered = gatherSourceValues(events, mSourceKey, S.kind, S.linePtr, S.lineLen);  // :121-129
    tally.outFailed = gathered.notLogEvent;
    tally.keyNotFound = gathered.noSourceKey;
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const uint32_t W = mFirstTripPairs ? mFirstTripPairs : kDefaultFirstTripPairs;
    // the first matched date-form line whose seconds format did not consume 19 bytes: behind it the cache is observable
    uint32_t replayFrom = UINT32_MAX;
    if (nLines) {
        const lc_apsara_out_t out = S.first.resize(nLines, W);
        int rc = lc_apsara_parse_host(S.linePtr.data(), S.lineLen.data(), nLines, W, &out);
        if (rc == LC_OK) {
            for (uint32_t li = 0; li < nLines && replayFrom == UINT32_MAX; ++li)
                if ((S.first.status[li] & (LC_APSARA_TIME_OK | LC_APSARA_EPOCH | LC_APSARA_CANON19)) == LC_APSARA_TIME_OK && S.lineLen[li]) replayFrom = li;
            // a line whose time failed is never stitched -- unless the replay gives it a cached one
            S.wanted.resize(nLines);
            for (uint32_t li = 0; li < nLines; ++li) S.wanted[li] = ((S.first.status[li] & LC_APSARA_TIME_OK) || li > replayFrom) ? 1 : 0;
            rc = runSecondTrip(S.linePtr, S.lineLen, S.wanted.data(), 1, S.first.npairs.data(), W, [&](uint32_t li) { return S.first.npairs[li]; },
                               T, mMopUpLinesTotal, [&](const SecondTrip& t) {
                                   const uint32_t n2 = uint32_t(t.linePtr.size());
                                   const lc_apsara_out_t out2 = S.second.resize(n2, t.W);
                                   return lc_apsara_parse_host(t.linePtr.data(), t.lineLen.data(), n2, t.W, &out2);
                               });
        }
        if (rc != LC_OK) {
            mOutFailedEventsTotal += tally.outFailed;
            mOutKeyNotFoundEventsTotal += tally.keyNotFound;
            return ReportFailedTrip(sName, "Apsara parse", "unparsed", rc, nLines);
        }
    }
    const int64_t now = Now();
    // the replay's state: cachedTimeStr / cachedLogTime (:92-93)
    const uint8_t* cache = nullptr;
    int64_t cacheSec = 0;
    uint64_t replayed = 0;
    size_t line = 0;
    compactEvents(events, [&](size_t i) {
        if (S.kind[i] != kToParse) return true;
        const uint32_t li = uint32_t(line++);
        const uint8_t* val = S.linePtr[li];
        const uint32_t len = S.lineLen[li];
        if (len == 0) {  // :132-135
            ++tally.outFailed;
            return true;
        }
        LogEvent& ev = events[i].Cast<LogEvent>();
        const StringView raw(reinterpret_cast<const char*>(val), len);
        const Results& R = S.first;
        // ---- ApsaraEasyReadLogTimeParser :251-323
        int64_t logTime = 0;
        uint32_t nsec = 0;
        if (li < replayFrom) {
            // (the cache, were it kept, would answer what the full path answers)
            if (R.status[li] & LC_APSARA_TIME_OK) {
                logTime = (R.status[li] & LC_APSARA_EPOCH) ? R.secs[li] : lc_timestamp_zone_seconds(R.secs[li], 0) - mLogTimeZoneOffsetSecond;
                nsec = R.nanos[li];
                if (!(R.status[li] & LC_APSARA_EPOCH)) {
                    cache = len > kCachedTimeBytes ? val + 1 : nullptr;
                    cacheSec = logTime;
                }
            }
        } else if (val[0] == '[') {
            ++replayed;
            const uint32_t n = timeTextLength(val, len);  // the text is val[1 .. n], its last byte the ']'
            const ApsaraHostSource host(val, len, 0);
            const ApsaraTimeView<ApsaraHostSource> view{host, 1};
            if (n == 0) {
                // :262-266, :279-283: no ']'
            } else if (val[1] == '1') {  // :259-276: the epoch form does not look at the cache
                uint8_t st = 0;
                int64_t secs = 0;
                apsaraTime(view, n, st, secs, nsec);
                if (st & LC_APSARA_TIME_OK) logTime = secs;
                else nsec = 0;
            } else if (cache && n >= kCachedTimeBytes && std::memcmp(val + 1, cache, kCachedTimeBytes) == 0) {  // :287-299
                uint32_t q = kCachedTimeBytes + 1;
                int32_t digits = 0;
                (void)tsConvNanos(view, n, q, nsec, digits);
                logTime = cacheSec;
            } else {  // :301-321
                uint8_t st = 0;
                int64_t secs = 0;
                apsaraTime(view, n, st, secs, nsec);
                if (st & LC_APSARA_TIME_OK) {
                    logTime = lc_timestamp_zone_seconds(secs, 0) - mLogTimeZoneOffsetSecond;
                    cache = len > kCachedTimeBytes ? val + 1 : nullptr;
                    cacheSec = logTime;
                } else {
                    nsec = 0;
                }
            }
        }
        const int64_t microTime = logTime * 1000000 + int64_t(nsec) / 1000;
        const size_t shown = len > 1024 ? 1024 : len;
        if (logTime <= 0) {  // :138-172
            RaiseAlarm(0, std::string(raw.data(), shown) + " $ " + std::to_string(logTime));
            ++tally.outFailed;
            return FinishSourceKey(ev, raw, false, false, mCommonParserOptions, metadata, tally);
        }
        if (mDiscardOldData && (now - logTime) > mDiscardInterval) {  // :173-199
            RaiseAlarm(1, "logTime: " + std::to_string(logTime) + ", log:" + std::string(raw.data(), shown));
            ++mHistoryFailureTotal;
            ++tally.discarded;
            return false;
        }
        ev.SetTimestamp(time_t(logTime), uint32_t(microTime * 1000 % 1000000000));  // :201
        // ---- ParseApsaraBaseFields :443-461: the fields as the line has them, one behind the other
        const int32_t* B = &R.base[size_t(li) * 8];
        struct Field {
            int32_t at;
            int kind;
        } order[3];
        int nf = 0;
        for (int k = 0; k < 3; ++k)
            if (B[2 * k] >= 0) order[nf++] = Field{k == LC_APSARA_FILE && B[2 * LC_APSARA_LINE] >= 0 ? B[2 * LC_APSARA_LINE + 1] : B[2 * k + 1], k};
        std::sort(order, order + nf, [](const Field& a, const Field& b) { return a.at < b.at; });
        for (int f = 0; f < nf; ++f) {
            const int k = order[f].kind;
            const std::string& key = k == LC_APSARA_LEVEL ? SLS_KEY_LEVEL : k == LC_APSARA_THREAD ? SLS_KEY_THREAD : SLS_KEY_FILE;
            appendContent(ev, StringView(key), StringView(raw.data() + B[2 * k], size_t(B[2 * k + 1] - B[2 * k])));
            if (k == LC_APSARA_FILE && B[2 * LC_APSARA_LINE] >= 0)
                appendContent(ev, StringView(SLS_KEY_LINE), StringView(raw.data() + B[6], size_t(B[7] - B[6])));
        }
        // ---- the pairs :202-224
        const uint32_t l2 = T.second[li];
        const uint32_t np = R.npairs[li];
        const int32_t* P = l2 != UINT32_MAX ? &S.second.pairs[size_t(l2) * T.W * 3] : &R.pairs[size_t(li) * W * 3];
        bool sourceKeyOverwritten = false;
        for (uint32_t k = 0; k < np; ++k) {
            const StringView key(raw.data() + P[3 * k], size_t(P[3 * k + 1] - P[3 * k]));
            appendContent(ev, key, StringView(raw.data() + P[3 * k + 1] + 1, size_t(P[3 * k + 2] - P[3 * k + 1] - 1)));
            if (key == StringView(mSourceKey)) sourceKeyOverwritten = true;
        }
        // ---- microtime :226-232
        StringBuffer sb = ev.GetSourceBuffer()->AllocateStringBuffer(20);
        sb.size = size_t(std::min(20, std::snprintf(sb.data, sb.capacity, "%ld", long(microTime))));
        appendContent(ev, StringView(kMicrotimeKey), StringView(sb.data, sb.size));
        ++tally.outSuccessful;
        return FinishSourceKey(ev, raw, true, sourceKeyOverwritten, mCommonParserOptions, metadata, tally);  // :233-240
    });
    AddTally(tally);
    mReplayedLines += replayed;
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_apsara.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseApsaraGpu;

struct lc_apsara_processor : logtail::ProcessorHandle<ProcessorParseApsaraGpu> {};

extern "C" int lc_apsara_processor_create(const char* config_json, lc_apsara_processor_t** out, char* err, size_t errcap) {
    return lc_apsara_processor_create_with_clock(config_json, nullptr, nullptr, out, err, errcap);
}
extern "C" int lc_apsara_processor_create_with_clock(const char* config_json, lc_clock_t clock, void* clock_user, lc_apsara_processor_t** out,
                                                     char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap, [&](lc_apsara_processor& h, const lcjson::Value& cfg, std::string& error) {
        h.impl.SetClock(clock, clock_user);  // Init resolves Timezone against it
        return h.impl.Init(cfg, error) ? int(LC_OK) : int(LC_ERR_SYNTAX);
    });
}
extern "C" void lc_apsara_processor_destroy(lc_apsara_processor_t* p) { delete p; }
extern "C" char* lc_apsara_processor_warnings(const lc_apsara_processor_t* p) { return logtail::warningsText(p); }
extern "C" int32_t lc_apsara_processor_zone_offset(const lc_apsara_processor_t* p) { return p ? p->impl.mLogTimeZoneOffsetSecond : 0; }
extern "C" int lc_apsara_processor_process_native(lc_apsara_processor_t* p, void* native_group) { return logtail::processNative(p, native_group); }
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_apsara_processor_process(lc_apsara_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" void lc_apsara_processor_set_clock(lc_apsara_processor_t* p, lc_clock_t clock, void* user) {
    if (p) p->impl.SetClock(clock, user);
}
extern "C" void lc_apsara_processor_set_discard(lc_apsara_processor_t* p, int discard_old_data, int32_t interval_seconds) {
    if (!p) return;
    p->impl.mDiscardOldData = discard_old_data != 0;
    p->impl.mDiscardInterval = interval_seconds;
}
extern "C" void lc_apsara_processor_set_first_trip_pairs(lc_apsara_processor_t* p, uint32_t pairs) {
    if (p) p->impl.mFirstTripPairs = pairs;
}
extern "C" int lc_apsara_processor_counters(const lc_apsara_processor_t* p, uint64_t out[LC_CNT_COUNT]) { return logtail::fillCounters(p, out, true); }
extern "C" uint64_t lc_apsara_processor_history_failures(const lc_apsara_processor_t* p) { return p ? uint64_t(p->impl.mHistoryFailureTotal) : 0; }
extern "C" void lc_apsara_processor_replayed_lines(const lc_apsara_processor_t* p, uint64_t out[2]) {
    if (!p || !out) return;
    out[0] = p->impl.mReplayedLines;
    out[1] = p->impl.mMopUpLinesTotal;
}
extern "C" void lc_apsara_processor_set_alarm_sink(lc_apsara_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_parse_apsara_gpu)
extern "C" int lcApsaraSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_apsara_processor_create, ProcessorParseApsaraGpu::sName, config_text, state);
}
extern "C" void lcApsaraSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_apsara_processor_t*>(state), native_group);
}
extern "C" void lcApsaraSlotFinalize(void* state) { delete static_cast<lc_apsara_processor_t*>(state); }
