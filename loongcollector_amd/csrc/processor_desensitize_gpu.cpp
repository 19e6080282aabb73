// processor_desensitize_gpu.cpp -- see processor_desensitize_gpu.hpp.
#include "processor_desensitize_gpu.hpp"

#include <cstdlib>
#include <cstring>

namespace logtail {

const std::string ProcessorDesensitizeGpu::sName = "processor_desensitize_gpu";

namespace {
// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<const uint8_t*> valuePtr, linePtr;  // every SourceKey value; the non-empty ones, which make the trip
    std::vector<uint32_t> valueLen, lineLen, lineEvent;
    std::vector<uint8_t> kind, flags;
    std::vector<uint64_t> outOff;
};
}  // namespace

// ProcessorDesensitizeNative::Init :28-144
bool ProcessorDesensitizeGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    if (!mandatoryString(config, "SourceKey", mSourceKey, error)) return false;
    std::string method;
    if (!mandatoryString(config, "Method", method, error)) return false;
    if (method == "const") {
        mMethod = LC_DESENS_CONST;
    } else if (method == "md5") {
        mMethod = LC_DESENS_MD5;
    } else {
        error = "string param Method is not valid";
        return false;
    }
    if (mMethod == LC_DESENS_CONST && !mandatoryString(config, "ReplacingString", mReplacingString, error)) return false;
    if (!mandatoryString(config, "ContentPatternBeforeReplacedString", mContentPatternBeforeReplacedString, error)) return false;
    if (!mandatoryString(config, "ReplacedContentPattern", mReplacedContentPattern, error)) return false;
    std::string warning;
    if (!optionalBool(config, "ReplacingAll", mReplacingAll, warning)) mInitWarnings.push_back(warning);
    char err[256] = "";
    int passThrough = 0;
    const int rc = lc_desens_create(mMethod, mContentPatternBeforeReplacedString.data(), mContentPatternBeforeReplacedString.size(),
                                    mReplacedContentPattern.data(), mReplacedContentPattern.size(), mReplacingString.data(), mReplacingString.size(),
                                    mReplacingAll ? 1 : 0, &mEngine, &passThrough, err, sizeof err);
    if (rc != LC_OK) {
        error = std::string("param ContentPatternBeforeReplacedString or ReplacedContentPattern is not a valid regex: ") + err;
        return false;
    }
    if (passThrough)
        mInitWarnings.push_back("param ReplacingString holds a backslash in front of something that is neither a digit nor a backslash: "
                                "values pass through unchanged");
    return true;
}

// Process :146-157 + ProcessEvent :159-196, restructured as gather -> device trip -> stitch
int ProcessorDesensitizeGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    S.linePtr.clear();
    S.lineLen.clear();
    S.lineEvent.clear();
    Tally tally;
    const Gathered gathered = gatherSourceValues(events, mSourceKey, S.kind, S.valuePtr, S.valueLen);
    tally.outFailed = gathered.notLogEvent + gathered.noSourceKey;  // :160-163, :192-194
    size_t value = 0;
    for (size_t i = 0; i < events.size(); ++i) {
        if (S.kind[i] != kToParse) continue;
        const size_t vi = value++;
        if (S.valueLen[vi] == 0) {  // :178-180, :190-191: only non-empty fields are processed
            ++tally.keyNotFound;
            continue;
        }
        ++tally.outSuccessful;
        S.linePtr.push_back(S.valuePtr[vi]);
        S.lineLen.push_back(S.valueLen[vi]);
        S.lineEvent.push_back(uint32_t(i));
    }
    const uint32_t nLines = uint32_t(S.linePtr.size());
    if (!nLines) {
        AddTally(tally);
        return LC_OK;
    }
    S.flags.resize(nLines);
    S.outOff.resize(size_t(nLines) + 1);
    uint8_t* bytes = nullptr;
    lc_desens_stats_t stats{};
    const int rc = lc_desens_apply_host(mEngine, S.linePtr.data(), S.lineLen.data(), nLines, S.flags.data(), S.outOff.data(), &bytes, &stats);
    if (rc != LC_OK) return ReportFailedTrip(sName, "desensitize", "untouched: do not forward the group", rc, nLines);
    mRoundsTotal += stats.rounds;
    const uint64_t total = S.outOff[nLines];
    if (total) {
        // the group's new bytes: one copy into its SourceBuffer; the changed events point into it
        SourceBuffer& buffer = *logGroup.GetSourceBuffer();
        const StringBuffer store = buffer.AllocateStringBuffer(size_t(total));
        std::memcpy(store.data, bytes, size_t(total));
        const StringBuffer key = buffer.CopyString(mSourceKey);
        const StringView keyView(key.data, key.size);
        for (uint32_t li = 0; li < nLines; ++li) {
            if (!(S.flags[li] & LC_DESENS_CHANGED)) continue;
            LogEvent& ev = events[S.lineEvent[li]].Cast<LogEvent>();
            ev.SetContentNoCopy(keyView, StringView(store.data + S.outOff[li], size_t(S.outOff[li + 1] - S.outOff[li])));
        }
    }
    std::free(bytes);
    uint64_t gaveUp = 0;
    for (uint32_t li = 0; li < nLines; ++li) {
        if (!(S.flags[li] & LC_DESENS_GAVE_UP)) continue;
        ++gaveUp;
        RaiseAlarm(1, "desensitize: the search gave up on event " + std::to_string(S.lineEvent[li]) + "; the value is left unchanged");
    }
    if (gaveUp) mComplexityExceededEventsTotal += gaveUp;
    AddTally(tally);
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_desensitize.h)
using logtail::ProcessorDesensitizeGpu;

struct lc_desensitize : logtail::ProcessorHandle<ProcessorDesensitizeGpu> {};

extern "C" int lc_desensitize_create(const char* config_json, lc_desensitize_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_desensitize_destroy(lc_desensitize_t* p) { delete p; }
extern "C" char* lc_desensitize_warnings(const lc_desensitize_t* p) { return logtail::warningsText(p); }
extern "C" int lc_desensitize_process_native(lc_desensitize_t* p, void* native_group) { return logtail::processNative(p, native_group); }
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_desensitize_process(lc_desensitize_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" int lc_desensitize_counters(const lc_desensitize_t* p, uint64_t out[LC_CNT_COUNT]) {
    const int rc = logtail::fillCounters(p, out, true);
    if (rc == LC_OK) out[LC_CNT_COMPLEXITY_EXCEEDED] = p->impl.mComplexityExceededEventsTotal;
    return rc;
}
extern "C" void lc_desensitize_set_alarm_sink(lc_desensitize_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}
extern "C" lc_desens_t* lc_desensitize_engine(const lc_desensitize_t* p) { return p ? p->impl.mEngine : nullptr; }
extern "C" uint64_t lc_desensitize_rounds(const lc_desensitize_t* p) { return p ? uint64_t(p->impl.mRoundsTotal) : 0; }

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_desensitize_gpu)
extern "C" int lcDesensitizeSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_desensitize_create, ProcessorDesensitizeGpu::sName, config_text, state);
}
extern "C" void lcDesensitizeSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_desensitize_t*>(state), native_group);
}
extern "C" void lcDesensitizeSlotFinalize(void* state) { delete static_cast<lc_desensitize_t*>(state); }
