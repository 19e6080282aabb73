// processor_parse_delimiter_gpu.cpp -- see processor_parse_delimiter_gpu.hpp.
#include "processor_parse_delimiter_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace logtail {

const std::string ProcessorParseDelimiterGpu::sName = "processor_parse_delimiter_gpu";
const std::string ProcessorParseDelimiterGpu::s_mDiscardedFieldKey = "_";

namespace {
// GetMandatoryStringParam / GetOptional*Param / GetMandatoryListParam (core/common/ParamExtractor.cpp:31-43,101-113,174-188,
// ParamExtractor.h:162-342)
bool mandatoryString(const lcjson::Value& cfg, const std::string& key, std::string& out, std::string& err) {
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
bool optionalString(const lcjson::Value& cfg, const std::string& key, std::string& out, std::string& err) {
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
bool optionalBool(const lcjson::Value& cfg, const std::string& key, bool& out, std::string& err) {
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

// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> kind, status, status2;
    std::vector<const uint8_t*> linePtr, linePtr2;
    std::vector<uint32_t> lineLen, lineLen2, ncols, ncols2, second;
    std::vector<int32_t> spans, spans2;
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
    // Keys :111-126
    {
        const lcjson::Value* keys = config.find("Keys");
        if (!keys) {
            error = "mandatory param Keys is missing";
            return false;
        }
        if (!keys->isArray()) {
            error = "param Keys is not of type list";
            return false;
        }
        mKeys.clear();
        for (const auto& k : keys->arr) {
            if (!k.isString()) {
                error = "element in list param Keys is not of type string";
                return false;
            }
            mKeys.push_back(k.str);
        }
        if (mKeys.empty()) {
            error = "mandatory list param Keys is empty";
            return false;
        }
    }
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

// :411-419
void ProcessorParseDelimiterGpu::AddLog(const StringView& key, const StringView& value, LogEvent& targetEvent, bool overwritten) {
    if (!overwritten && targetEvent.HasContent(key)) return;
    targetEvent.SetContentNoCopy(key, value);
}

void ProcessorParseDelimiterGpu::RaiseAlarm(int kind, const std::string& message) const {
    if (mAlarmSink) mAlarmSink(mAlarmUser, kind, message.data(), message.size());
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
    // :350-363
    if (!parseSuccess || !mSourceKeyOverwritten) ev.DelContent(mSourceKey);
    if (mCommonParserOptions.ShouldAddSourceContent(parseSuccess)) AddLog(mCommonParserOptions.mRenamedSourceKey, raw, ev, false);
    if (mCommonParserOptions.ShouldAddLegacyUnmatchedRawLog(parseSuccess))
        AddLog(GpuCommonParserOptions::legacyUnmatchedRawLogKey, raw, ev, false);
    if (mCommonParserOptions.ShouldEraseEvent(parseSuccess, ev, metadata)) {
        ++tally.discarded;
        return false;
    }
    return true;
}

// Process :186-204 + ProcessEvent :206-282, restructured as gather -> device trip(s) -> stitch
int ProcessorParseDelimiterGpu::Process(PipelineEventGroup& logGroup) {
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
    Tally tally;
    for (size_t i = 0; i < nEvents; ++i) {
        PipelineEventPtr& e = events[i];
        if (!e.Is<LogEvent>()) {  // :209-212
            ++tally.outFailed;
            continue;
        }
        LogEvent& ev = e.Cast<LogEvent>();
        if (!ev.HasContent(mSourceKey)) {  // :214-217
            ++tally.keyNotFound;
            continue;
        }
        const StringView raw = ev.GetContent(mSourceKey);
        S.kind[i] = Parse;
        S.linePtr.push_back(reinterpret_cast<const uint8_t*>(raw.data()));
        S.lineLen.push_back(uint32_t(raw.size()));
    }
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const size_t K = mKeys.size();
    const bool extend = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::EXTEND;
    // the reference's reserve (:244-245): the first trip keeps this many columns per line
    const uint32_t W = mFirstTripColumns ? mFirstTripColumns : uint32_t(extend ? K + 10 : K + 1);
    // what the stitch reads of a line with n columns: all of them, except in discard mode (the keys' columns only, :335-337)
    const bool discard = mOverflowedFieldsTreatment == OverflowedFieldsTreatment::DISCARD;
    uint32_t W2 = 0;
    if (nLines) {
        S.status.resize(nLines);
        S.ncols.resize(nLines);
        S.spans.resize(size_t(nLines) * W * 2);
        int rc = lc_delim_split_host(mDelim, S.linePtr.data(), S.lineLen.data(), nLines, W, S.status.data(), S.ncols.data(), S.spans.data());
        S.second.assign(nLines, UINT32_MAX);
        if (rc == LC_OK) {
            // the mop-up: the kernel always reports the TRUE count, so the lines that did not fit take ONE second trip with room for
            // the widest of them
            S.linePtr2.clear();
            S.lineLen2.clear();
            for (uint32_t li = 0; li < nLines; ++li) {
                const uint32_t needed = discard && S.ncols[li] > K ? uint32_t(K) : S.ncols[li];
                if (S.status[li] == LC_DELIM_OK && needed > W) {
                    S.second[li] = uint32_t(S.linePtr2.size());
                    S.linePtr2.push_back(S.linePtr[li]);
                    S.lineLen2.push_back(S.lineLen[li]);
                    W2 = S.ncols[li] > W2 ? S.ncols[li] : W2;
                }
            }
            if (!S.linePtr2.empty()) {
                const uint32_t n2 = uint32_t(S.linePtr2.size());
                S.status2.resize(n2);
                S.ncols2.resize(n2);
                S.spans2.resize(size_t(n2) * W2 * 2);
                rc = lc_delim_split_host(mDelim, S.linePtr2.data(), S.lineLen2.data(), n2, W2, S.status2.data(), S.ncols2.data(), S.spans2.data());
                mMopUpLinesTotal += n2;
            }
        }
        if (rc != LC_OK) {
            // no CPU path: the events stay exactly as they came in, and the failure is said loudly
            const std::string message = "GPU split failed (rc=" + std::to_string(rc) + ": " + lc_last_error() + "); " + std::to_string(nLines) +
                                        " events left unparsed";
            if (mAlarmSink) RaiseAlarm(3, message);
            else std::fprintf(stderr, "[%s] %s\n", sName.c_str(), message.c_str());
            mDeviceFailedEventsTotal += nLines;
            mOutFailedEventsTotal += tally.outFailed;
            mOutKeyNotFoundEventsTotal += tally.keyNotFound;
            return rc;
        }
    }
    // stitch + in-place compaction (:193-202)
    size_t wIdx = 0, line = 0;
    for (size_t rIdx = 0; rIdx < nEvents; ++rIdx) {
        bool keep = true;
        if (S.kind[rIdx] == Parse) {
            const size_t li = line++;
            LogEvent& ev = events[rIdx].Cast<LogEvent>();
            const StringView raw(reinterpret_cast<const char*>(S.linePtr[li]), S.lineLen[li]);
            if (S.status[li] == LC_DELIM_BLANK) {
                ++tally.outFailed;  // :220-224, :239-242: nothing behind the trim -- counted, and the event goes on as it came
            } else if (S.second[li] != UINT32_MAX) {
                const uint32_t l2 = S.second[li];
                keep = FinishEvent(ev, raw, S.status2[l2], S.ncols2[l2], &S.spans2[size_t(l2) * W2 * 2], metadata, tally);
            } else {
                keep = FinishEvent(ev, raw, S.status[li], S.ncols[li], &S.spans[li * W * 2], metadata, tally);
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

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_delimiter.h)
using logtail::PipelineEventGroup;
using logtail::ProcessorParseDelimiterGpu;

struct lc_delimiter_processor {
    ProcessorParseDelimiterGpu impl;
    // what ProcessorInstance adds around every plugin (ProcessorInstance.cpp:46-63)
    std::atomic<uint64_t> inEvents{0}, outEvents{0}, inBytes{0}, outBytes{0};
};

extern "C" int lc_delimiter_processor_create(const char* config_json, lc_delimiter_processor_t** out, char* err, size_t errcap) {
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
    auto p = std::make_unique<lc_delimiter_processor>();
    std::string error;
    if (!p->impl.Init(cfg, error)) {
        setErr(error);
        return LC_ERR_SYNTAX;
    }
    setErr("");
    *out = p.release();
    return LC_OK;
}
extern "C" void lc_delimiter_processor_destroy(lc_delimiter_processor_t* p) { delete p; }
extern "C" char* lc_delimiter_processor_warnings(const lc_delimiter_processor_t* p) {
    std::string s;
    if (p)
        for (const std::string& w : p->impl.mInitWarnings) s += w + "\n";
    char* out = static_cast<char*>(std::malloc(s.size() + 1));
    if (out) std::memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
extern "C" int lc_delimiter_processor_process_native(lc_delimiter_processor_t* p, void* native_group) {
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
extern "C" int lc_delimiter_processor_process(lc_delimiter_processor_t* p, lc_event_group_t* group) {
    if (!p || !group) return LC_ERR_ARG;
    return lc_delimiter_processor_process_native(p, lc_group_native(group));
}
#endif
extern "C" void lc_delimiter_processor_set_first_trip_columns(lc_delimiter_processor_t* p, uint32_t columns) {
    if (p) p->impl.mFirstTripColumns = columns;
}
extern "C" int lc_delimiter_processor_counters(const lc_delimiter_processor_t* p, uint64_t out[LC_CNT_COUNT]) {
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
extern "C" void lc_delimiter_processor_set_alarm_sink(lc_delimiter_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_parse_delimiter_gpu)
extern "C" int lcDelimiterSlotInit(const char* config_text, void** state) {
    lc_delimiter_processor_t* p = nullptr;
    char err[256];
    if (lc_delimiter_processor_create(config_text, &p, err, sizeof err) != LC_OK) {
        std::fprintf(stderr, "[processor_parse_delimiter_gpu] init failed: %s\n", err);
        return -1;
    }
    *state = p;
    return 0;
}
extern "C" void lcDelimiterSlotProcess(void* state, void* native_group) {
    (void)lc_delimiter_processor_process_native(static_cast<lc_delimiter_processor_t*>(state), native_group);
}
extern "C" void lcDelimiterSlotFinalize(void* state) { lc_delimiter_processor_destroy(static_cast<lc_delimiter_processor_t*>(state)); }
