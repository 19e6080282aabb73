// processor_parse_prom_gpu.cpp -- see processor_parse_prom_gpu.hpp.
#include "processor_parse_prom_gpu.hpp"

#include <charconv>
#include <cstring>

#include "prom_vm.hpp"
#ifdef LC_USE_REFERENCE_HEADERS
#include "models/MetricEvent.h"
#include "models/RawEvent.h"
#endif

namespace logtail {

const std::string ProcessorParsePromGpu::sName = "processor_prom_parse_metric_gpu";

namespace {
const std::string kNameTag = "__name__";  // prometheus::NAME (core/prometheus/Constants.h)

// one runner thread's scratch for Process()
struct ProcessScratch {
    std::vector<uint8_t> status, flags;
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen, nanos, nlabels;
    std::vector<int32_t> name, valueSpan, timeSpan;
    std::vector<uint64_t> value;
    std::vector<int64_t> secs;
    // (16-byte vectors on the device; the host entry copies into it with memcpy)
    std::vector<int32_t> labels;
    void resize(uint32_t n, uint32_t W) {
        status.resize(n);
        flags.resize(n);
        nanos.resize(n);
        nlabels.resize(n);
        name.resize(size_t(n) * 2);
        valueSpan.resize(size_t(n) * 2);
        timeSpan.resize(size_t(n) * 2);
        value.resize(n);
        secs.resize(n);
        labels.resize(size_t(n) * W * 4);
    }
    lc_prom_out_t out() {
        return lc_prom_out_t{status.data(), flags.data(), name.data(), value.data(), valueSpan.data(), timeSpan.data(), secs.data(), nanos.data(),
                             nlabels.data(), labels.data()};
    }
};

bool allDigits(const std::string& s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; }  // IsNumber (Utils.cpp:128)
bool zeroNumber(const std::string& s) { return s.find_first_not_of('0') == std::string::npos; }
// DurationToSecond (core/prometheus/Utils.cpp:36-48) == 0
bool durationIsZero(const std::string& d) {
    if (d.size() <= 1 || !allDigits(d.substr(0, d.size() - 1))) return true;
    if (d.back() != 's' && d.back() != 'm') return true;
    return zeroNumber(d.substr(0, d.size() - 1));
}
// SizeToByte (Utils.cpp:51-110) == 0: the unit is found by the text's end, the number is what stands in front of the unit's FIRST letter
bool sizeIsZero(const std::string& s) {
    if (s.empty()) return true;
    for (const char unit : std::string("KMGTPE")) {
        const std::string u(1, unit);
        const auto endsWith = [&](const std::string& tail) { return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0; };
        if (endsWith(u + "iB") || endsWith(u) || endsWith(u + "B")) {
            const std::string number = s.substr(0, s.find(unit));
            return !allDigits(number) || zeroNumber(number);
        }
    }
    if (s.back() == 'B') {
        const std::string number = s.substr(0, s.find('B'));
        return !allDigits(number) || zeroNumber(number);
    }
    return true;
}

#ifdef LC_USE_REFERENCE_HEADERS
void pushMetric(EventsContainer& out, std::unique_ptr<MetricEvent>&& e) { out.emplace_back(std::move(e), true, nullptr); }
#else
void pushMetric(EventsContainer& out, std::unique_ptr<MetricEvent>&& e) { out.emplace_back(std::move(e)); }
#endif
}  // namespace

// ProcessorPromParseMetricNative::Init :19-25 -> ScrapeConfig::InitStaticConfig (ScrapeConfig.cpp:116-214)
bool ProcessorParsePromGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!config.isObject()) {
        error = "plugin config is not an object";
        return false;
    }
    const lcjson::Value* job = config.find("job_name");
    if (!job || !job->isString()) {  // :117-125
        error = "job_name is missing or not a string";
        return false;
    }
    mJobName = job->str;
    if (mJobName.empty()) {
        error = "job name is empty";
        return false;
    }
    const lcjson::Value* v = nullptr;
    if ((v = config.find("scrape_interval")) && v->isString() && durationIsZero(v->str)) {  // :127-134
        error = "scrape interval is invalid: " + v->str;
        return false;
    }
    if ((v = config.find("scrape_timeout")) && v->isString() && durationIsZero(v->str)) {  // :135-142
        error = "scrape timeout is invalid: " + v->str;
        return false;
    }
    if ((v = config.find("honor_timestamps")) && v->isBool()) mHonorTimestamps = v->b;  // :151-153 (another type: the default stays)
    if ((v = config.find("max_scrape_size")) && v->isString() && sizeIsZero(v->str)) {  // :160-167
        error = "max scrape size is invalid: " + v->str;
        return false;
    }
    // relabel_configs, metric_relabel_configs, external_labels, host_only_mode: accepted and ignored (lc_prom.h)
    return true;
}

// Process :27-46 + ProcessEvent :52-66, restructured as gather -> device trip(s) -> build
int ProcessorParsePromGpu::Process(PipelineEventGroup& eGroup) {
    EventsContainer& events = eGroup.MutableEvents();
    if (events.empty()) return LC_OK;
    static thread_local ProcessScratch tFirst, tSecond;
    ProcessScratch& S = tFirst;
    S.linePtr.clear();
    S.lineLen.clear();
    for (const PipelineEventPtr& e : events) {
        if (!e.Is<RawEvent>()) continue;
        const StringView content = e.Cast<RawEvent>().GetContent();
        S.linePtr.push_back(reinterpret_cast<const uint8_t*>(content.data()));
        S.lineLen.push_back(uint32_t(content.size()));
    }
    const uint32_t nLines = uint32_t(S.linePtr.size());
    const uint32_t W = mFirstTripLabels ? mFirstTripLabels : 1u;
    SecondTrip second;
    if (nLines) {
        S.resize(nLines, W);
        const lc_prom_out_t out = S.out();
        uint64_t deferred = 0;
        int rc = lc_prom_parse_host(mHonorTimestamps ? 1 : 0, S.linePtr.data(), S.lineLen.data(), nLines, &out, W, &deferred);
        if (rc == LC_OK) {
            rc = runSecondTrip(S.linePtr, S.lineLen, S.status.data(), uint8_t(LC_PROM_OK), S.nlabels.data(), W, [&](uint32_t li) { return S.nlabels[li]; },
                               second, mMopUpLinesTotal, [&](SecondTrip& T) {
                                   tSecond.resize(uint32_t(T.linePtr.size()), T.W);
                                   const lc_prom_out_t again = tSecond.out();
                                   // (the tokens of these lines were finished and counted by the first trip)
                                   return lc_prom_parse_host(mHonorTimestamps ? 1 : 0, T.linePtr.data(), T.lineLen.data(), uint32_t(T.linePtr.size()), &again,
                                                             T.W, nullptr);
                               });
        }
        if (rc != LC_OK) return ReportFailedTrip(sName, "Prometheus line parse", "unparsed", rc, nLines);
        if (deferred) mDeferredTokens += deferred;
    }
    // :32-38: the default timestamp (StringTo<uint64_t>: std::from_chars over the whole text)
    const StringView scrapeText = eGroup.GetMetadata(EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC);
    uint64_t scrapeMs = 0;
    {
        const char* first = scrapeText.data();
        const char* last = first + scrapeText.size();
        const auto conv = first && first < last ? std::from_chars(first, last, scrapeMs) : std::from_chars_result{first, std::errc::invalid_argument};
        if (conv.ec != std::errc() || conv.ptr != last) {
            scrapeMs = 0;
            RaiseAlarm(1, "parse scrape timestamp failed: " + scrapeText.to_string() + "\tprocessor: " + sName + "\tconfig: " + mConfigName);
        }
    }
    const time_t defaultSecs = time_t(scrapeMs / 1000);
    const uint32_t defaultNanos = uint32_t(scrapeMs % 1000 * 1000000);

    Tally tally;
    EventsContainer newEvents;
    newEvents.reserve(nLines);
    std::string unescaped;
    uint32_t li = 0;
    for (PipelineEventPtr& e : events) {
        if (!e.Is<RawEvent>()) {  // :56-58: not taken over into the new container
            ++tally.discarded;
            continue;
        }
        const uint32_t line = li++;
        if (S.status[line] != LC_PROM_OK) {  // :61: no event (the reference logs a warning, no alarm)
            ++tally.outFailed;
            continue;
        }
        const uint8_t* bytes = S.linePtr[line];
        const char* text = reinterpret_cast<const char*>(bytes);
        std::unique_ptr<MetricEvent> metric = eGroup.CreateMetricEvent(true);
        const StringView name(text + S.name[size_t(line) * 2], size_t(S.name[size_t(line) * 2 + 1] - S.name[size_t(line) * 2]));
        metric->SetNameNoCopy(name);
        const uint32_t at = second.second.empty() ? UINT32_MAX : second.second[line];
        const int32_t* labels = at == UINT32_MAX ? &S.labels[size_t(line) * W * 4] : &tSecond.labels[size_t(at) * second.W * 4];
        for (uint32_t k = 0; k < S.nlabels[line]; ++k) {
            const int32_t* l = labels + size_t(k) * 4;
            const StringView key(text + l[0], size_t(l[1] - l[0]));
            const int32_t vb = int32_t(uint32_t(l[2]) & ~LC_PROM_LABEL_ESCAPED), ve = l[3];
            if (uint32_t(l[2]) & LC_PROM_LABEL_ESCAPED) {  // :209-211
                promUnescape(bytes, vb, ve, unescaped);
                metric->SetTag(key.to_string(), unescaped);
            } else {  // :207-208
                metric->SetTagNoCopy(key, StringView(text + vb, size_t(ve - vb)));
            }
        }
        double value = 0;
        std::memcpy(&value, &S.value[line], 8);
        metric->SetValue<UntypedSingleValue>(value);
        if (S.flags[line] & LC_PROM_HAS_TIME) metric->SetTimestamp(time_t(S.secs[line]), S.nanos[line]);
        else metric->SetTimestamp(defaultSecs, defaultNanos);
        metric->SetTag(kNameTag, name.to_string());  // :62
        pushMetric(newEvents, std::move(metric));
        ++tally.outSuccessful;
    }
    events.swap(newEvents);  // :45
    AddTally(tally);
    return LC_OK;
}

}  // namespace logtail

// ---------------------------------------------------------------------------------------------- C ABI (include/lc_prom.h)
using logtail::ProcessorParsePromGpu;

struct lc_prom_processor : logtail::ProcessorHandle<ProcessorParsePromGpu> {};

extern "C" int lc_prom_processor_create(const char* config_json, lc_prom_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_prom_processor_destroy(lc_prom_processor_t* p) { delete p; }
extern "C" char* lc_prom_processor_warnings(const lc_prom_processor_t* p) { return logtail::warningsText(p); }
extern "C" void lc_prom_processor_set_config_name(lc_prom_processor_t* p, const char* name) {
    if (p) p->impl.mConfigName = name ? name : "";
}
extern "C" int lc_prom_processor_process_native(lc_prom_processor_t* p, void* native_group) { return logtail::processNative(p, native_group); }
#ifndef LC_USE_REFERENCE_HEADERS
extern "C" void* lc_group_native(lc_event_group_t* g);
extern "C" int lc_prom_processor_process(lc_prom_processor_t* p, lc_event_group_t* group) {
    return p && group ? logtail::processNative(p, lc_group_native(group)) : LC_ERR_ARG;
}
#endif
extern "C" int lc_prom_processor_counters(const lc_prom_processor_t* p, uint64_t out[LC_CNT_COUNT]) { return logtail::fillCounters(p, out, true); }
extern "C" uint64_t lc_prom_processor_deferred_tokens(const lc_prom_processor_t* p) { return p ? uint64_t(p->impl.mDeferredTokens) : 0; }
extern "C" uint64_t lc_prom_processor_mop_up_lines(const lc_prom_processor_t* p) { return p ? uint64_t(p->impl.mMopUpLinesTotal) : 0; }
extern "C" void lc_prom_processor_set_first_trip_labels(lc_prom_processor_t* p, uint32_t W) {
    if (p) p->impl.mFirstTripLabels = W;
}
extern "C" void lc_prom_processor_set_alarm_sink(lc_prom_processor_t* p, lc_alarm_sink_t sink, void* user) {
    if (p) p->impl.SetAlarmSink(sink, user);
}

// ---- the plugin slot's way to this processor (c_processor_slot.cpp: a config whose Type is processor_prom_parse_metric_gpu)
extern "C" int lcPromSlotInit(const char* config_text, void** state) {
    return logtail::slotInitHandle(&lc_prom_processor_create, ProcessorParsePromGpu::sName, config_text, state);
}
extern "C" void lcPromSlotProcess(void* state, void* native_group) {
    (void)logtail::processNative(static_cast<lc_prom_processor_t*>(state), native_group);
}
extern "C" void lcPromSlotFinalize(void* state) { delete static_cast<lc_prom_processor_t*>(state); }
