// processor_parse_delimiter_gpu.cpp -- see processor_parse_delimiter_gpu.hpp.
#include "processor_parse_delimiter_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace logtail {

const std::string ProcessorParseDelimiterGpu::sName = "processor_parse_delimiter_gpu";
const std::string ProcessorParseDelimiterGpu::s_mDiscardedFieldKey = "_";

namespace {
// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> kind, status, status2;
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen, ncols, ncols2;
    std::vector<int32_t> spans, spans2;
    SecondTrip mopUp;
};
}  // namespace

ProcessorParseDelimiterGpu::~ProcessorParseDelimiterGpu() {
    if (mDelim) lc_delim_destroy(mDelim);
}

// ProcessorParseDelimiterNative::Init :30-184
bool ProcessorParseDelimiterGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    std::string err;
    if (!mandatoryString(config, "SourceKey", mSourceKey, error)) return false;  // :33-43
    if (!mandatoryString(config, "Separator", mSeparator, error)) return false;  // :45-55
    if (mSeparator.size() > 4) {                                                 // :56-65
        error = "mandatory string param Separator has more than 4 chars";
        return false;
    }
    if (mSeparator == "\\t") mSeparator = "\t";  // :66-69
    mSeparatorChar = mSeparator[0];
    // Quote :72-107
    std::string quoteStr;
    const bool res = optionalString(config, "Quote", quoteStr, err);
    if (mSeparator.size() == 1) {
        if (!res) {
            mInitWarnings.push_back(err);  // (the default '"' stays)
        } else if (quoteStr.size() > 1) {
            error = "string param Quote is not a single char";
            return false;
        } else if (!quoteStr.empty()) {
            mQuote = quoteStr[0];
        }
    } else if (!quoteStr.empty()) {
        mInitWarnings.push_back("string param Quote is not allowed when param Separator is not a single char");
    }
    if (!mandatoryStringList(config, "Keys", "element in list param Keys is not of type string", mKeys, error)) return false;  // :111-126
    mSourceKeyOverwritten = false;
    for (const auto& key : mKeys)
        if (key == mSourceKey) mSourceKeyOverwritten = true;
    // :128-139
    if (!optionalBool(config, "AllowingShortenedFields", mAllowingShortenedFields, err)) mInitWarnings.push_back(err);
    // :141-167
    std::string treatment;
    if (!optionalString(config, "OverflowedFieldsTreatment", treatment, err)) {
        mInitWarnings.push_back(err);
    } else if (treatment == "keep") {
        mOverflowedFieldsTreatment = OverflowedFieldsTreatment::KEEP;
    } else if (treatment == "discard") {
        mOverflowedFieldsTreatment = OverflowedFieldsTreatment::DISCARD;
    } else if (!treatment.empty() && treatment != "extend") {
        mInitWarnings.push_back("string param OverflowedFieldsTreatment is not valid");
    }
    mExtractingPartialFields = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::DISCARD;  // :169-172
    if (!mCommonParserOptions.Init(config, mInitWarnings)) return false;                          // :174
    mUseQuote = mSeparator.size() == 1 && mQuote != mSeparatorChar;  // :251
    const int mode = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::EXTEND ? LC_DELIM_EXTEND
                     : mOverflowedFieldsTreatment == OverflowedFieldsTreatment::KEEP ? LC_DELIM_KEEP : LC_DELIM_DISCARD;
    if (lc_delim_create(reinterpret_cast<const uint8_t*>(mSeparator.data()), uint32_t(mSeparator.size()), uint8_t(mQuote), mode,
                        uint32_t(mKeys.size()), &mDelim) != LC_OK) {
        error = "the delimiter engine refused the separator";
        return false;
    }
    return true;
}

StringView ProcessorParseDelimiterGpu::ColumnValue(LogEvent& ev, StringView raw, int32_t begin, int32_t end) const {
    const uint32_t b = uint32_t(begin) & ~LC_DELIM_DOUBLED, e = uint32_t(end);
    if (!(uint32_t(begin) & LC_DELIM_DOUBLED)) return StringView(raw.data() + b, e - b);
    // AddFieldWithUnQuote :94-111: a pair of quotes becomes one; a quote that is not followed by another one is dropped
    StringBuffer sb = ev.GetSourceBuffer()->AllocateStringBuffer(e - b);
    size_t j = 0;
    for (uint32_t i = b; i < e; ++i) {
        if (raw[i] == mQuote) {
            if (i + 1 < e && raw[i + 1] == mQuote) {
                sb.data[j++] = mQuote;
                ++i;
            }
        } else {
            sb.data[j++] = raw[i];
        }
    }
    return StringView(sb.data, j);
}

// ProcessEvent :244-363 behind the split
bool ProcessorParseDelimiterGpu::FinishEvent(LogEvent& ev, StringView raw, uint8_t status, uint32_t ncols, const int32_t* spans,
                                             const GroupMetadata& metadata, Tally& tally) {
    bool parseSuccess = status == LC_DELIM_OK;
    size_t parsedColCount = ncols;
    StringView joined;  // keep / discard on the quote path: the columns behind the keys, re-joined (:258-275)
    const size_t K = mKeys.size();
    if (K == 0) {  // :312-323 (Init refuses an empty list: kept for a caller that fills mKeys itself)
        RaiseAlarm(4, "no column keys defined");
        parseSuccess = false;
    } else if (parseSuccess) {
        if (mUseQuote && mOverflowedFieldsTreatment != OverflowedFieldsTreatment::EXTEND && ncols > K) {
            if (mOverflowedFieldsTreatment == OverflowedFieldsTreatment::KEEP) {
                // (the un-quoted values, each behind a separator byte; DISCARD never reads it)
                std::vector<StringView> rest;
                size_t requiredLen = 0;
                for (size_t i = K; i < ncols; ++i) {
                    rest.push_back(ColumnValue(ev, raw, spans[2 * i], spans[2 * i + 1]));
                    requiredLen += 1 + rest.back().size();
                }
                StringBuffer sb = ev.GetSourceBuffer()->AllocateStringBuffer(requiredLen);
                char* at = sb.data;
                for (const StringView& v : rest) {
                    *at++ = mSeparatorChar;
                    std::memcpy(at, v.data(), v.size());
                    at += v.size();
                }
                joined = StringView(sb.data, requiredLen);
            }
            parsedColCount = K + 1;
        }
        if (parsedColCount == 0 || (!mAllowingShortenedFields && parsedColCount < K)) {  // :285-301
            RaiseAlarm(2, "keys count unmatch columns count :" + std::to_string(parsedColCount) + ", required:" + std::to_string(K) +
                              ", logs:" + std::string(raw.data(), raw.size()));
            parseSuccess = false;
        }
    } else {  // :302-311
        RaiseAlarm(0, "parse delimiter log fail, logs:" + std::string(raw.data(), raw.size()));
    }

    if (parseSuccess) {  // :325-345
        for (uint32_t idx = 0; idx < parsedColCount; ++idx) {
            if (K > idx) {
                if (mExtractingPartialFields && mKeys[idx] == s_mDiscardedFieldKey) continue;
                AddLog(StringView(mKeys[idx]), ColumnValue(ev, raw, spans[2 * idx], spans[2 * idx + 1]), ev);
            } else {
                if (mExtractingPartialFields) continue;
                const std::string key = "__column" + std::to_string(idx) + "__";
                StringBuffer sb = ev.GetSourceBuffer()->CopyString(key);
                const bool isJoined = mUseQuote && mOverflowedFieldsTreatment == OverflowedFieldsTreatment::KEEP && idx == K;
                AddLog(StringView(sb.data, sb.size), isJoined ? joined : ColumnValue(ev, raw, spans[2 * idx], spans[2 * idx + 1]), ev);
            }
        }
        ++tally.outSuccessful;
    } else {
        ++tally.outFailed;
    }
    return FinishSourceKey(ev, raw, parseSuccess, mSourceKeyOverwritten, mCommonParserOptions, metadata, tally);  // :350-363
}

// Process :186-204 + ProcessEvent :206-282, restructured as gather -> device trip(s) -> stitch
int ProcessorParseDelimiterGpu::Process(PipelineEventGroup& logGroup) {
    if (logGroup.GetEvents().empty()) return LC_OK;
    EventsContainer& events = logGroup.MutableEvents();
    const GroupMetadata& metadata = logGroup.GetAllMetadata();
    static thread_local ProcessScratch tScratch;
    ProcessScratch& S = tScratch;
    SecondTrip& T = S.mopUp;
    Tally tally;
    const Gathered gathered = gatherSourceValues(events, mSourceKey, S.kind, S.linePtr, S.lineLen);  // :209-217
    tally.outFailed = gathered.notLogEvent;
    tally.keyNotFound = gathered.noSourceKey;
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const size_t K = mKeys.size();
    const bool extend = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::EXTEND;
    // the reference's reserve (:244-245): the first trip keeps this many columns per line
    const uint32_t W = mFirstTripColumns ? mFirstTripColumns : uint32_t(extend ? K + 10 : K + 1);
    // what the stitch reads of a line with n columns: all of them, except in discard mode (the keys' columns only, :335-337)
    const bool discard = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::DISCARD;
    if (nLines) {
        S.status.resize(nLines);
        S.ncols.resize(nLines);
        S.spans.resize(size_t(nLines) * W * 2);
        int rc = lc_delim_split_host(mDelim, S.linePtr.data(), S.lineLen.data(), nLines, W, S.status.data(), S.ncols.data(), S.spans.data());
        if (rc == LC_OK)
            rc = runSecondTrip(S.linePtr, S.lineLen, S.status.data(), LC_DELIM_OK, S.ncols.data(), W,
                               [&](uint32_t li) { return discard && S.ncols[li] > K ? uint32_t(K) : S.ncols[li]; }, T, mMopUpLinesTotal,
                               [&](const SecondTrip& t) {
                                   const uint32_t n2 = uint32_t(t.linePtr.size());
                                   S.status2.resize(n2);
                                   S.ncols2.resize(n2);
                                   S.spans2.resize(size_t(n2) * t.W * 2);
                                   return lc_delim_split_host(mDelim, t.linePtr.data(), t.lineLen.data(), n2, t.W, S.status2.data(),
                                                              S.ncols2.data(), S.spans2.data());
                               });
        if (rc != LC_OK) {
            mOutFailedEventsTotal += tally.outFailed;
            mOutKeyNotFoundEventsTotal += tally.keyNotFound;
            return ReportFailedTrip(sName, "split", "unparsed", rc, nLines);
        }
    }
    // stitch + in-place compaction (:193-202)
    size_t line = 0;
    compactEvents(events, [&](size_t i) {
        if (S.kind[i] != kToParse) return true;
        const size_t li = line++;
        LogEvent& ev = events[i].Cast<LogEvent>();
        const StringView raw(reinterpret_cast<const char*>(S.linePtr[li]), S.lineLen[li]);
        if (S.status[li] == LC_DELIM_BLANK) {
            ++tally.outFailed;  // :220-224, :239-242: nothing behind the trim -- counted, and the event goes on as it came
            return true;
        }
        const uint32_t l2 = T.second[li];
        if (l2 != UINT32_MAX) return FinishEvent(ev, raw, S.status2[l2], S.ncols2[l2], &S.spans2[size_t(l2) * T.W * 2], metadata, tally);
        return FinishEvent(ev, raw, S.status[li], S.ncols[li], &S.spans[li * W * 2], metadata, tally);
    });
    AddTally(tally);
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_delimiter.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseDelimiterGpu;

struct lc_delimiter_processor : logtail::ProcessorHandle<ProcessorParseDelimiterGpu> {};

extern "C" int lc_delimiter_processor_create(const char* config_json, lc_delimiter_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_delimiter_processor_destroy(lc_delimiter_processor_t* p) { delete p; }
extern "C" char* lc_delimiter_processor_warnings(const lc_delimiter_processor_t* p) { return logtail::warningsText(p); }
extern "C" int lc_delimiter_processor_process_native(lc_delimiter_processor_t* p, void* native_group) {
    return logtail::processNative(p, native_group);
}
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_delimiter_processor_process(lc_delimiter_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" void lc_delimiter_processor_set_first_trip_columns(lc_delimiter_processor_t* p, uint32_t columns) {
    if (p) p->impl.mFirstTripColumns = columns;
}
extern "C" int lc_delimiter_processor_counters(const lc_delimiter_processor_t* p, uint64_t out[LC_CNT_COUNT]) {
    return logtail::fillCounters(p, out, true);
}
extern "C" void lc_delimiter_processor_set_alarm_sink(lc_delimiter_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_parse_delimiter_gpu)
extern "C" int lcDelimiterSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_delimiter_processor_create, ProcessorParseDelimiterGpu::sName, config_text, state);
}
extern "C" void lcDelimiterSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_delimiter_processor_t*>(state), native_group);
}
extern "C" void lcDelimiterSlotFinalize(void* state) { delete static_cast<lc_delimiter_processor_t*>(state); }
