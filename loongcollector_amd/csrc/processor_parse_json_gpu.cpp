// processor_parse_json_gpu.cpp -- see processor_parse_json_gpu.hpp.
#include "processor_parse_json_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace logtail {

const std::string ProcessorParseJsonGpu::sName = "processor_parse_json_gpu";

namespace {
// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> kind, status, status2, shadow, shadow2;
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen, nmembers, nmembers2, errpos, errpos2;
    std::vector<size_t> shadowAt, shadowAt2;
    std::vector<lc_json_member_t> records, records2;
    SecondTrip mopUp;
};
}  // namespace

// ProcessorParseJsonNative::Init :44-84
bool ProcessorParseJsonGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    if (!mandatoryString(config, "SourceKey", mSourceKey, error)) return false;  // :48-57
    return mCommonParserOptions.Init(config, mInitWarnings);                     // :59-61
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
    if (!FinishSourceKey(ev, raw, parseSuccess, sourceKeyOverwritten, mCommonParserOptions, metadata, tally)) return false;  // :130-144
    ++tally.outSuccessful;  // (:143: every event that goes on, parsed or not)
    return true;
}

// Process :87-105 + ProcessEvent :107-128, restructured as gather -> device trip(s) -> stitch
int ProcessorParseJsonGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    const GroupMetadata& metadata = logGroup.GetAllMetadata();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    SecondTrip& T = S.mopUp;
    Tally tally;
    const Gathered gathered = gatherSourceValues(events, mSourceKey, S.kind, S.linePtr, S.lineLen);  // :110-118
    tally.outFailed = gathered.notLogEvent;
    tally.keyNotFound = gathered.noSourceKey;
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const uint32_t W = mFirstTripMembers ? mFirstTripMembers : 32u;  // :309
    if (nLines) {
        S.status.resize(nLines);
        S.nmembers.resize(nLines);
        S.errpos.resize(nLines);
        S.records.resize(size_t(nLines) * W);
        S.shadow.resize(prefixSums(S.lineLen, S.shadowAt) + 1);
        uint64_t moved = 0, moved2 = 0;
        int rc = lc_json_walk_host(S.linePtr.data(), S.lineLen.data(), nLines, W, S.status.data(), S.nmembers.data(), S.errpos.data(),
                                   S.records.data(), S.shadow.data(), &moved);
        if (rc == LC_OK)
            rc = runSecondTrip(S.linePtr, S.lineLen, S.status.data(), LC_JSON_OK, S.nmembers.data(), W, [&](uint32_t li) { return S.nmembers[li]; },
                               T, mMopUpLinesTotal, [&](const SecondTrip& t) {
                                   const uint32_t n2 = uint32_t(t.linePtr.size());
                                   S.status2.resize(n2);
                                   S.nmembers2.resize(n2);
                                   S.errpos2.resize(n2);
                                   S.records2.resize(size_t(n2) * t.W);
                                   S.shadow2.resize(prefixSums(t.lineLen, S.shadowAt2) + 1);
                                   return lc_json_walk_host(t.linePtr.data(), t.lineLen.data(), n2, t.W, S.status2.data(), S.nmembers2.data(),
                                                            S.errpos2.data(), S.records2.data(), S.shadow2.data(), &moved2);
                               });
        if (rc != LC_OK) {
            mOutFailedEventsTotal += tally.outFailed;
            mOutKeyNotFoundEventsTotal += tally.keyNotFound;
            return ReportFailedTrip(sName, "JSON walk", "unparsed", rc, nLines);
        }
        mShadowBytesTotal += moved + moved2;
    }
    // stitch + in-place compaction (:95-104)
    size_t line = 0;
    compactEvents(events, [&](size_t i) {
        if (S.kind[i] != kToParse) return true;
        const size_t li = line++;
        LogEvent& ev = events[i].Cast<LogEvent>();
        const StringView raw(reinterpret_cast<const char*>(S.linePtr[li]), S.lineLen[li]);
        const uint32_t l2 = T.second[li];
        if (l2 != UINT32_MAX)
            return FinishEvent(ev, raw, S.status2[l2], S.nmembers2[l2], &S.records2[size_t(l2) * T.W], S.shadow2.data() + S.shadowAt2[l2], metadata, tally);
        return FinishEvent(ev, raw, S.status[li], S.nmembers[li], &S.records[li * W], S.shadow.data() + S.shadowAt[li], metadata, tally);
    });
    AddTally(tally);
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_json.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseJsonGpu;

struct lc_json_processor : logtail::ProcessorHandle<ProcessorParseJsonGpu> {};

extern "C" int lc_json_processor_create(const char* config_json, lc_json_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_json_processor_destroy(lc_json_processor_t* p) { delete p; }
extern "C" char* lc_json_processor_warnings(const lc_json_processor_t* p) { return logtail::warningsText(p); }
extern "C" int lc_json_processor_process_native(lc_json_processor_t* p, void* native_group) { return logtail::processNative(p, native_group); }
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_json_processor_process(lc_json_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" void lc_json_processor_set_first_trip_members(lc_json_processor_t* p, uint32_t members) {
    if (p) p->impl.mFirstTripMembers = members;
}
extern "C" int lc_json_processor_counters(const lc_json_processor_t* p, uint64_t out[LC_CNT_COUNT]) { return logtail::fillCounters(p, out, true); }
extern "C" void lc_json_processor_set_alarm_sink(lc_json_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}
