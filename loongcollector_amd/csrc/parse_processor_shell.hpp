// parse_processor_shell.hpp -- what processor_parse_delimiter_gpu, processor_parse_timestamp_gpu, processor_parse_json_gpu, processor_parse_apsara_gpu and processor_parse_container_log_gpu share around
// their own Init, engine call and stitch: the config readers, the counters / alarm sink / tally every parse processor holds, the gather,
// the ONE second trip for lines wider than the first trip kept, the report of a failed trip, the source-key tail, the in-place
// compaction, and the C ABI bodies as templates over the handle type.  Header-only; it uses only the event API the stand-in and the
// reference's event model both offer (HasContent, GetContent, SetContentNoCopy, DelContent, Is / Cast, MutableEvents).
#pragma once

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc_processor.h"
#include "processor_parse_regex_gpu.hpp"  // the event model, json_min, GpuCommonParserOptions

namespace logtail {

// ---------------------------------------------------------------------------------------------- config readers
// GetMandatoryStringParam / GetOptional*Param / GetMandatoryListParam (core/common/ParamExtractor.cpp:31-43,101-113,174-188,
// ParamExtractor.h:162-342)
inline bool mandatoryString(const lcjson::Value& cfg, const std::string& key, std::string& out, std::string& err) {
    const lcjson::Value* v = cfg.find(key);
    if (!v) {
        err = "mandatory param " + key + " is missing";
        return false;
    }
    if (!v->isString()) {
        err = "param " + key + " is not of type string";
        return false;
    }
    out = v->str;
    if (out.empty()) {
        err = "mandatory string param " + key + " is empty";
        return false;
    }
    return true;
}
inline bool optionalString(const lcjson::Value& cfg, const std::string& key, std::string& out, std::string& err) {
    const lcjson::Value* v = cfg.find(key);
    if (v) {
        if (!v->isString()) {
            err = "param " + key + " is not of type string";
            return false;
        }
        out = v->str;
    }
    return true;
}
inline bool optionalBool(const lcjson::Value& cfg, const std::string& key, bool& out, std::string& err) {
    const lcjson::Value* v = cfg.find(key);
    if (v) {
        if (!v->isBool()) {
            err = "param " + key + " is not of type bool";
            return false;
        }
        out = v->b;
    }
    return true;
}
// a mandatory, non-empty list of strings; elementMessage: the whole text for an element that is no string (the two readers of the
// reference word it differently)
inline bool mandatoryStringList(const lcjson::Value& cfg, const std::string& key, const char* elementMessage, std::vector<std::string>& out,
                                std::string& err) {
    const lcjson::Value* list = cfg.find(key);
    if (!list) {
        err = "mandatory param " + key + " is missing";
        return false;
    }
    if (!list->isArray()) {
        err = "param " + key + " is not of type list";
        return false;
    }
    out.clear();
    for (const auto& k : list->arr) {
        if (!k.isString()) {
            err = elementMessage;
            return false;
        }
        out.push_back(k.str);
    }
    if (out.empty()) {
        err = "mandatory list param " + key + " is empty";
        return false;
    }
    return true;
}

// std::from_chars<int> over exactly two bytes (StringTo of core/common/StringTools.h)
inline bool twoCharInt(const char* s, int& out) {
    const bool neg = s[0] == '-';
    if (neg) {
        if (s[1] < '0' || s[1] > '9') return false;
        out = -(s[1] - '0');
        return true;
    }
    if (s[0] < '0' || s[0] > '9' || s[1] < '0' || s[1] > '9') return false;
    out = (s[0] - '0') * 10 + (s[1] - '0');
    return true;
}
// ParseTimeZoneOffsetSecond (TimeUtil.cpp:407-426)
inline bool parseTimeZoneOffsetSecond(const std::string& tz, int& out) {
    if (tz.size() != 9 || tz[6] != ':' || (tz[3] != '+' && tz[3] != '-')) return false;
    if (tz.compare(0, 3, "GMT") != 0) return false;
    int hour = 0, minute = 0;
    if (!twoCharInt(tz.data() + 4, hour) || !twoCharInt(tz.data() + 7, minute)) return false;
    out = hour * 3600 + minute * 60;
    if (tz[3] == '-') out = -out;
    return true;
}

// ---------------------------------------------------------------------------------------------- what every parse processor holds
struct ParseProcessorBase {
    std::string mSourceKey;
    // plugin counters
    std::atomic<uint64_t> mDiscardedEventsTotal{0}, mOutFailedEventsTotal{0}, mOutKeyNotFoundEventsTotal{0}, mOutSuccessfulEventsTotal{0};
    std::atomic<uint64_t> mDeviceFailedEventsTotal{0};  // no reference counterpart: events passed on unparsed behind a failed trip
    std::vector<std::string> mInitWarnings;

    using AlarmSink = void (*)(void* user, int kind, const char* message, size_t len);
    void SetAlarmSink(AlarmSink sink, void* user) {
        mAlarmSink = sink;
        mAlarmUser = user;
    }

protected:
    // per-call tallies: the runner threads share the instance; Process() adds its tally to the counters once, at the end
    struct Tally {
        uint64_t discarded = 0, outFailed = 0, keyNotFound = 0, outSuccessful = 0;
    };
    void AddTally(const Tally& tally) {
        if (tally.discarded) mDiscardedEventsTotal += tally.discarded;
        if (tally.outFailed) mOutFailedEventsTotal += tally.outFailed;
        if (tally.keyNotFound) mOutKeyNotFoundEventsTotal += tally.keyNotFound;
        if (tally.outSuccessful) mOutSuccessfulEventsTotal += tally.outSuccessful;
    }
    static void AddLog(const StringView& key, const StringView& value, LogEvent& targetEvent, bool overwritten = true) {
        if (!overwritten && targetEvent.HasContent(key)) return;
        targetEvent.SetContentNoCopy(key, value);
    }
    void RaiseAlarm(int kind, const std::string& message) const {
        if (mAlarmSink) mAlarmSink(mAlarmUser, kind, message.data(), message.size());
    }
    // A failed device trip.  There is no CPU path: the events stay exactly as they came in, and the failure is said loudly -- alarm
    // kind 3 to the sink, without one a line on stderr: "GPU <what> failed (rc=..: ..); N events left <left>".  Returns rc.
    int ReportFailedTrip(const std::string& name, const char* what, const char* left, int rc, uint32_t nLines) {
        const std::string message = std::string("GPU ") + what + " failed (rc=" + std::to_string(rc) + ": " + lc_last_error() + "); " +
                                    std::to_string(nLines) + " events left " + left;
        if (mAlarmSink) RaiseAlarm(3, message);
        else std::fprintf(stderr, "[%s] %s\n", name.c_str(), message.c_str());
        mDeviceFailedEventsTotal += nLines;
        return rc;
    }
    // the tail of the reference's ProcessEvent: the source key is dropped, renamed or kept, the legacy raw log added, and the event
    // erased if nothing is left of it.  false: erased (counted).  What counts as a success is the caller's.
    bool FinishSourceKey(LogEvent& ev, StringView raw, bool parseSuccess, bool sourceKeyOverwritten, const GpuCommonParserOptions& options,
                         const GroupMetadata& metadata, Tally& tally) const {
        if (!parseSuccess || !sourceKeyOverwritten) ev.DelContent(mSourceKey);
        if (options.ShouldAddSourceContent(parseSuccess)) AddLog(options.mRenamedSourceKey, raw, ev, false);
        if (options.ShouldAddLegacyUnmatchedRawLog(parseSuccess)) AddLog(GpuCommonParserOptions::legacyUnmatchedRawLogKey, raw, ev, false);
        if (options.ShouldEraseEvent(parseSuccess, ev, metadata)) {
            ++tally.discarded;
            return false;
        }
        return true;
    }

    AlarmSink mAlarmSink = nullptr;
    void* mAlarmUser = nullptr;
};

// ---------------------------------------------------------------------------------------------- gather, mop-up, compaction
enum GatherKind : uint8_t { kNotLogEvent, kNoSourceKey, kToParse };
struct Gathered {
    uint64_t notLogEvent = 0, noSourceKey = 0;
};
// kind[i] for every event; the source values of the kToParse ones, in order, as views into the group's SourceBuffer
inline Gathered gatherSourceValues(EventsContainer& events, const std::string& sourceKey, std::vector<uint8_t>& kind,
                                   std::vector<const uint8_t*>& linePtr, std::vector<uint32_t>& lineLen) {
    Gathered g;
    kind.assign(events.size(), kNotLogEvent);
    linePtr.clear();
    lineLen.clear();
    for (size_t i = 0; i < events.size(); ++i) {
        PipelineEventPtr& e = events[i];
        if (!e.Is<LogEvent>()) {
            ++g.notLogEvent;
            continue;
        }
        LogEvent& ev = e.Cast<LogEvent>();
        if (!ev.HasContent(sourceKey)) {
            kind[i] = kNoSourceKey;
            ++g.noSourceKey;
            continue;
        }
        const StringView raw = ev.GetContent(sourceKey);
        kind[i] = kToParse;
        linePtr.push_back(reinterpret_cast<const uint8_t*>(raw.data()));
        lineLen.push_back(uint32_t(raw.size()));
    }
    return g;
}
// at[i] = where line i starts when the lines lie back to back; returns their total length
inline size_t prefixSums(const std::vector<uint32_t>& len, std::vector<size_t>& at) {
    size_t total = 0;
    at.resize(len.size());
    for (size_t i = 0; i < len.size(); ++i) {
        at[i] = total;
        total += len[i];
    }
    return total;
}

// The mop-up: the kernels always report the TRUE count of a line, so the lines whose stitch needs more than the first trip's W take
// ONE second trip with room for the widest of them.
struct SecondTrip {
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen;
    std::vector<uint32_t> second;  // per first-trip line: its index in the second trip, UINT32_MAX: it did not take one
    uint32_t W = 0;
};
// needed(li): how many of line li's count[li] entries the stitch reads; trip(T): the engine call over T's lines at width T.W
template <class Needed, class Trip>
int runSecondTrip(const std::vector<const uint8_t*>& linePtr, const std::vector<uint32_t>& lineLen, const uint8_t* status, uint8_t okStatus,
                  const uint32_t* count, uint32_t W, Needed needed, SecondTrip& T, std::atomic<uint64_t>& mopUpLinesTotal, Trip trip) {
    const uint32_t nLines = uint32_t(linePtr.size());
    T.linePtr.clear();
    T.lineLen.clear();
    T.second.assign(nLines, UINT32_MAX);
    T.W = 0;
    for (uint32_t li = 0; li < nLines; ++li) {
        if (status[li] == okStatus && needed(li) > W) {
            T.second[li] = uint32_t(T.linePtr.size());
            T.linePtr.push_back(linePtr[li]);
            T.lineLen.push_back(lineLen[li]);
            T.W = count[li] > T.W ? count[li] : T.W;
        }
    }
    if (T.linePtr.empty()) return LC_OK;
    const int rc = trip(T);
    mopUpLinesTotal += T.linePtr.size();
    return rc;
}

// in-place compaction: keep(i) finishes event i and says whether it stays
template <class Keep>
void compactEvents(EventsContainer& events, Keep keep) {
    const size_t nEvents = events.size();
    size_t wIdx = 0;
    for (size_t rIdx = 0; rIdx < nEvents; ++rIdx) {
        if (keep(rIdx)) {
            if (wIdx != rIdx) events[wIdx] = std::move(events[rIdx]);
            ++wIdx;
        }
    }
    events.resize(wIdx);
}

// ---------------------------------------------------------------------------------------------- the C ABI bodies
// a processor and what ProcessorInstance adds around every plugin (ProcessorInstance.cpp:46-63)
template <class Processor>
struct ProcessorHandle {
    Processor impl;
    std::atomic<uint64_t> inEvents{0}, outEvents{0}, inBytes{0}, outBytes{0};
};

inline void setErrorText(char* err, size_t errcap, const std::string& m) {
    if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
}
template <class Handle>
int initHandle(Handle& h, const lcjson::Value& cfg, std::string& error) {
    return h.impl.Init(cfg, error) ? LC_OK : LC_ERR_SYNTAX;
}
// *_create: init(handle, config, error) -> LC_OK or the LC_ERR_* code of the refusal; it is the place for what has to happen before Init
template <class Handle, class Init = int (*)(Handle&, const lcjson::Value&, std::string&)>
int createHandle(const char* config_json, Handle** out, char* err, size_t errcap, Init init = &initHandle<Handle>) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    lcjson::Value cfg;
    try {
        cfg = lcjson::parse(config_json);
    } catch (const std::exception& e) {
        setErrorText(err, errcap, e.what());
        return LC_ERR_ARG;
    }
    auto p = std::make_unique<Handle>();
    std::string error;
    const int rc = init(*p, cfg, error);
    setErrorText(err, errcap, error);
    if (rc == LC_OK) *out = p.release();
    return rc;
}
// *_warnings: one warning per line, malloc'ed
template <class Handle>
char* warningsText(const Handle* p) {
    std::string s;
    if (p)
        for (const std::string& w : p->impl.mInitWarnings) s += w + "\n";
    char* out = static_cast<char*>(std::malloc(s.size() + 1));
    if (out) std::memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
template <class Handle>
int processNative(Handle* p, void* native_group) {
    if (!p || !native_group) return LC_ERR_ARG;
    PipelineEventGroup& group = *static_cast<PipelineEventGroup*>(native_group);
    p->inEvents += group.GetEvents().size();
    p->inBytes += group.DataSize();
    const int rc = p->impl.Process(group);
    p->outEvents += group.GetEvents().size();
    p->outBytes += group.DataSize();
    return rc;
}
// *_counters: the entries every processor has; zeroFirst: the others are answered as 0 (lc_processor_counters fills them itself)
template <class Handle>
int fillCounters(const Handle* p, uint64_t out[LC_CNT_COUNT], bool zeroFirst) {
    if (!p || !out) return LC_ERR_ARG;
    if (zeroFirst)
        for (int i = 0; i < LC_CNT_COUNT; ++i) out[i] = 0;
    out[LC_CNT_DISCARDED_EVENTS] = p->impl.mDiscardedEventsTotal;
    out[LC_CNT_OUT_FAILED_EVENTS] = p->impl.mOutFailedEventsTotal;
    out[LC_CNT_OUT_KEY_NOT_FOUND] = p->impl.mOutKeyNotFoundEventsTotal;
    out[LC_CNT_OUT_SUCCESSFUL_EVENTS] = p->impl.mOutSuccessfulEventsTotal;
    out[LC_CNT_IN_EVENTS] = p->inEvents;
    out[LC_CNT_OUT_EVENTS] = p->outEvents;
    out[LC_CNT_IN_SIZE_BYTES] = p->inBytes;
    out[LC_CNT_OUT_SIZE_BYTES] = p->outBytes;
    out[LC_CNT_DEVICE_FAILED_EVENTS] = p->impl.mDeviceFailedEventsTotal;
    return LC_OK;
}
// the plugin slot's init for a processor type (c_processor_slot.cpp kSlotTable)
template <class Handle>
int slotInitHandle(int (*create)(const char*, Handle**, char*, size_t), const std::string& name, const char* config_text, void** state) {
    Handle* p = nullptr;
    char err[256];
    if (create(config_text, &p, err, sizeof err) != LC_OK) {
        std::fprintf(stderr, "[%s] init failed: %s\n", name.c_str(), err);
        return -1;
    }
    *state = p;
    return 0;
}

}  // namespace logtail
