// processor_parse_json_gpu.cpp -- see processor_parse_json_gpu.hpp.
#include "processor_parse_json_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace logtail {

const std::string ProcessorParseJsonGpu::sName = "processor_parse_json_gpu";

namespace {
// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> kind, status, status2, shadow, shadow2;
    std::vector<const uint8_t*> linePtr, linePtr2;
    std::vector<uint32_t> lineLen, lineLen2, nmembers, nmembers2, errpos, errpos2, second;
    std::vector<size_t> shadowAt, shadowAt2;
    std::vector<lc_json_member_t> records, records2;
};
}  // namespace

// ProcessorParseJsonNative::Init :44-84; GetMandatoryStringParam core/common/ParamExtractor.cpp:174-188
bool ProcessorParseJsonGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    const lcjson::Value* v = config.find("SourceKey");  // :48-57
    if (!v) {
        error = "mandatory param SourceKey is missing";
        return false;
    }
    if (!v->isString()) {
        error = "param SourceKey is not of type string";
        return false;
    }
    mSourceKey = v->str;
    if (mSourceKey.empty()) {
        error = "mandatory string param SourceKey is empty";
        return false;
    }
    return mCommonParserOptions.Init(config, mInitWarnings);  // :59-61
}

// :469-477
void ProcessorParseJsonGpu::AddLog(const StringView& key, const StringView& value, LogEvent& targetEvent, bool overwritten) {
    if (!overwritten && targetEvent.HasContent(key)) return;
    targetEvent.SetContentNoCopy(key, value);
}

void ProcessorParseJsonGpu::RaiseAlarm(int kind, const std::string& message) const {
    if (mAlarmSink) mAlarmSink(mAlarmUser, kind, message.data(), message.size());
}

// ProcessEvent :122-144 behind the parse; shadow: the line's own unescaped bytes
bool ProcessorParseJsonGpu::FinishEvent(LogEvent& ev, StringView raw, uint8_t status, uint32_t nmembers, const lc_json_member_t* members,
                                        const uint8_t* shadow, const GroupMetadata& metadata, Tally& tally) {
    const bool parseSuccess = status == LC_JSON_OK;
    bool sourceKeyOverwritten = false;
    if (parseSuccess) {
        auto text = [&](uint32_t begin, uint32_t end) {
            const uint32_t b = begin & ~LC_JSON_ESCAPED;
            if (!(begin & LC_JSON_ESCAPED)) return StringView(raw.data() + b, end - b);
            StringBuffer sb = ev.GetSourceBuffer()->CopyString(reinterpret_cast<const char*>(shadow + b), end - b);
            return StringView(sb.data, sb.size);
        };
        for (uint32_t k = 0; k < nmembers; ++k) {  // :316-350, :369-371
            const lc_json_member_t& m = members[k];
            const StringView key = text(m.key_begin, m.key_end);
            StringView value;
            switch (m.type) {
            case LC_JSON_STRING:
                value = text(m.val_begin, m.val_end);
                break;
            case LC_JSON_NULL:  // :194-198
                value = StringView(raw.data() + m.val_begin, 0);
                break;
            case LC_JSON_DOUBLE: {  // :175-181: std::to_string of the correctly rounded double
                char literal[64], out[400];
                const uint32_t n = m.val_end - m.val_begin;
                double d;
                if (n < sizeof literal) {
                    std::memcpy(literal, raw.data() + m.val_begin, n);
                    literal[n] = 0;
                    d = std::strtod(literal, nullptr);
                } else {
                    d = std::strtod(std::string(raw.data() + m.val_begin, n).c_str(), nullptr);
                }
                const int len = std::snprintf(out, sizeof out, "%f", d);
                StringBuffer sb = ev.GetSourceBuffer()->CopyString(out, size_t(len));
                value = StringView(sb.data, sb.size);
                break;
            }
            default:  // INT, TRUE, FALSE, OBJECT, ARRAY: the text as it stands in the line
                value = StringView(raw.data() + m.val_begin, m.val_end - m.val_begin);
                break;
            }
            if (key.size() == mSourceKey.size() && std::memcmp(key.data(), mSourceKey.data(), key.size()) == 0) sourceKeyOverwritten = true;
            AddLog(key, value, ev);
        }
    } else if (status == LC_JSON_FAIL) {  // :271-287 (an empty value fails without a counter and without an alarm, :259)
        RaiseAlarm(0, "parse json fail:" + std::string(raw.data(), raw.size()));
        ++tally.outFailed;
    }
    // :130-144
    if (!parseSuccess || !sourceKeyOverwritten) ev.DelContent(mSourceKey);
    if (mCommonParserOptions.ShouldAddSourceContent(parseSuccess)) AddLog(mCommonParserOptions.mRenamedSourceKey, raw, ev, false);
    if (mCommonParserOptions.ShouldAddLegacyUnmatchedRawLog(parseSuccess))
        AddLog(GpuCommonParserOptions::legacyUnmatchedRawLogKey, raw, ev, false);
    if (mCommonParserOptions.ShouldEraseEvent(parseSuccess, ev, metadata)) {
        ++tally.discarded;
        return false;
    }
    ++tally.outSuccessful;  // (:143: every event that goes on, parsed or not)
    return true;
}

// Process :87-105 + ProcessEvent :107-128, restructured as gather -> device trip(s) -> stitch
int ProcessorParseJsonGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    const GroupMetadata& metadata = logGroup.GetAllMetadata();
    const size_t nEvents = events.size();
    enum Kind : uint8_t { Keep, Parse };
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    S.kind.assign(nEvents, Keep);
    S.linePtr.clear();
    S.lineLen.clear();
    S.shadowAt.clear();
    Tally tally;
    size_t totalBytes = 0;
    for (size_t i = 0; i < nEvents; ++i) {
        PipelineEventPtr& e = events[i];
        if (!e.Is<LogEvent>()) {  // :110-113
            ++tally.outFailed;
            continue;
        }
        LogEvent& ev = e.Cast<LogEvent>();
        if (!ev.HasContent(mSourceKey)) {  // :115-118
            ++tally.keyNotFound;
            continue;
        }
        const StringView raw = ev.GetContent(mSourceKey);
        S.kind[i] = Parse;
        S.linePtr.push_back(reinterpret_cast<const uint8_t*>(raw.data()));
        S.lineLen.push_back(uint32_t(raw.size()));
        S.shadowAt.push_back(totalBytes);
        totalBytes += raw.size();
    }
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const uint32_t W = mFirstTripMembers ? mFirstTripMembers : 32u;  // :309
    uint32_t W2 = 0;
    if (nLines) {
        S.status.resize(nLines);
        S.nmembers.resize(nLines);
        S.errpos.resize(nLines);
        S.records.resize(size_t(nLines) * W);
        S.shadow.resize(totalBytes + 1);
        uint64_t moved = 0, moved2 = 0;
        int rc = lc_json_walk_host(S.linePtr.data(), S.lineLen.data(), nLines, W, S.status.data(), S.nmembers.data(), S.errpos.data(),
                                   S.records.data(), S.shadow.data(), &moved);
        S.second.assign(nLines, UINT32_MAX);
        if (rc == LC_OK) {
            // the mop-up: the kernel always reports the TRUE count, so the lines that did not fit take ONE second trip with room for
            // the one with the most members
            S.linePtr2.clear();
            S.lineLen2.clear();
            S.shadowAt2.clear();
            size_t bytes2 = 0;
            for (uint32_t li = 0; li < nLines; ++li) {
                if (S.status[li] == LC_JSON_OK && S.nmembers[li] > W) {
                    S.second[li] = uint32_t(S.linePtr2.size());
                    S.linePtr2.push_back(S.linePtr[li]);
                    S.lineLen2.push_back(S.lineLen[li]);
                    S.shadowAt2.push_back(bytes2);
                    bytes2 += S.lineLen[li];
                    W2 = S.nmembers[li] > W2 ? S.nmembers[li] : W2;
                }
            }
            if (!S.linePtr2.empty()) {
                const uint32_t n2 = uint32_t(S.linePtr2.size());
                S.status2.resize(n2);
                S.nmembers2.resize(n2);
                S.errpos2.resize(n2);
                S.records2.resize(size_t(n2) * W2);
                S.shadow2.resize(bytes2 + 1);
                rc = lc_json_walk_host(S.linePtr2.data(), S.lineLen2.data(), n2, W2, S.status2.data(), S.nmembers2.data(), S.errpos2.data(),
                                       S.records2.data(), S.shadow2.data(), &moved2);
                mMopUpLinesTotal += n2;
            }
        }
        if (rc != LC_OK) {
            // no CPU path: the events stay exactly as they came in, and the failure is said loudly
            const std::string message = "GPU JSON walk failed (rc=" + std::to_string(rc) + ": " + lc_last_error() + "); " + std::to_string(nLines) +
                                        " events left unparsed";
            if (mAlarmSink) RaiseAlarm(3, message);
            else std::fprintf(stderr, "[%s] %s\n", sName.c_str(), message.c_str());
            mDeviceFailedEventsTotal += nLines;
            mOutFailedEventsTotal += tally.outFailed;
            mOutKeyNotFoundEventsTotal += tally.keyNotFound;
            return rc;
        }
        mShadowBytesTotal += moved + moved2;
    }
    // stitch + in-place compaction (:95-104)
    size_t wIdx = 0, line = 0;
    for (size_t rIdx = 0; rIdx < nEvents; ++rIdx) {
        bool keep = true;
        if (S.kind[rIdx] == Parse) {
            const size_t li = line++;
            LogEvent& ev = events[rIdx].Cast<LogEvent>();
            const StringView raw(reinterpret_cast<const char*>(S.linePtr[li]), S.lineLen[li]);
            if (S.second[li] != UINT32_MAX) {
                const uint32_t l2 = S.second[li];
                keep = FinishEvent(ev, raw, S.status2[l2], S.nmembers2[l2], &S.records2[size_t(l2) * W2], S.shadow2.data() + S.shadowAt2[l2], metadata, tally);
            } else {
                keep = FinishEvent(ev, raw, S.status[li], S.nmembers[li], &S.records[li * W], S.shadow.data() + S.shadowAt[li], metadata, tally);
            }
        }
        if (keep) {
            if (wIdx != rIdx) events[wIdx] = std::move(events[rIdx]);
            ++wIdx;
        }
    }
    events.resize(wIdx);
    if (tally.discarded) mDiscardedEventsTotal += tally.discarded;
    if (tally.outFailed) mOutFailedEventsTotal += tally.outFailed;
    if (tally.keyNotFound) mOutKeyNotFoundEventsTotal += tally.keyNotFound;
    if (tally.outSuccessful) mOutSuccessfulEventsTotal += tally.outSuccessful;
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_json.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseJsonGpu;

struct lc_json_processor {
    ProcessorParseJsonGpu impl;
    // what ProcessorInstance adds around every plugin (ProcessorInstance.cpp:46-63)
    std::atomic<uint64_t> inEvents{0}, outEvents{0}, inBytes{0}, outBytes{0};
};

extern "C" int lc_json_processor_create(const char* config_json, lc_json_processor_t** out, char* err, size_t errcap) {
    if (!config_json || !out) return LC_ERR_ARG;
    *out = nullptr;
    auto setErr = [&](const std::string& m) {
        if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    };
    lcjson::Value cfg;
    try {
        cfg = lcjson::parse(config_json);
    } catch (const std::exception& e) {
        setErr(e.what());
        return LC_ERR_ARG;
    }
    auto p = std::make_unique<lc_json_processor>();
    std::string error;
    if (!p->impl.Init(cfg, error)) {
        setErr(error);
        return LC_ERR_SYNTAX;
    }
    setErr("");
    *out = p.release();
    return LC_OK;
}
extern "C" void lc_json_processor_destroy(lc_json_processor_t* p) { delete p; }
extern "C" char* lc_json_processor_warnings(const lc_json_processor_t* p) {
    std::string s;
    if (p)
        for (const std::string& w : p->impl.mInitWarnings) s += w + "\n";
    char* out = static_cast<char*>(std::malloc(s.size() + 1));
    if (out) std::memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
extern "C" int lc_json_processor_process_native(lc_json_processor_t* p, void* native_group) {
    if (!p || !native_group) return LC_ERR_ARG;
    PipelineEventGroup& group = *static_cast<PipelineEventGroup*>(native_group);
    p->inEvents += group.GetEvents().size();
    p->inBytes += group.DataSize();
    const int rc = p->impl.Process(group);
    p->outEvents += group.GetEvents().size();
    p->outBytes += group.DataSize();
    return rc;
}
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_json_processor_process(lc_json_processor_t* p, lc_event_group_t* group) {
    if (!p || !group) return LC_ERR_ARG;
    return lc_json_processor_process_native(p, lc_group_native(group));
}
#endif
extern "C" void lc_json_processor_set_first_trip_members(lc_json_processor_t* p, uint32_t members) {
    if (p) p->impl.mFirstTripMembers = members;
}
extern "C" int lc_json_processor_counters(const lc_json_processor_t* p, uint64_t out[LC_CNT_COUNT]) {
    if (!p || !out) return LC_ERR_ARG;
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
extern "C" void lc_json_processor_set_alarm_sink(lc_json_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}
