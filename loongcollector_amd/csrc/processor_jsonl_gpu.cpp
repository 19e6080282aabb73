// processor_jsonl_gpu.cpp -- the processor level of the JSON-lines encoder (include/jsonl/lc_jsonl.h): processor_parse_regex_native
// followed by JsonEventGroupSerializer, as one call that leaves the group alone.  The parser is ProcessorParseRegexGpu itself; what an
// event becomes is READ OFF that class by the probe events of parse_probe_items.hpp, as ProcessorSlsGpu does.  The head of every
// record is built per call from the group's tags (lc_jsonl_head).
// No HIP here: the tests build this file on a host double of lc_jsonl_match_encode_host.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/jsonl/lc_jsonl.h"
#include "jsonl_vm.hpp"
#include "parse_probe_items.hpp"
#include "parse_processor_shell.hpp"

namespace logtail {

class ProcessorJsonlGpu {
public:
    ~ProcessorJsonlGpu() { lc_jsonl_plan_free(mPlan); }
    bool Init(const lcjson::Value& config, std::string& error);
    int Serialize(PipelineEventGroup& group, const uint8_t** out, size_t* outLen, int* fused);

    ProcessorParseRegexGpu mParse;
    std::atomic<uint64_t> mGroupsDevice{0}, mGroupsHost{0}, mFailedTrips{0}, mBytes{0};

private:
    using Tally = ProcessorParseRegexGpu::Tally;
    bool DevicePathServes(const PipelineEventGroup& group) const;
    int SerializeOnDevice(PipelineEventGroup& group, const uint8_t** out, size_t* outLen, bool* undecided);
    void SerializeOnHost(PipelineEventGroup& group, const uint8_t** out, size_t* outLen);

    lc_jsonl_plan_t* mPlan = nullptr;  // null: no device path for this configuration
    Tally mFailedTally;                // what FinishEvent books for ONE line the parser did not match
};

namespace {
// one runner thread's scratch: the gather of the device path, the head, the bytes of the host path
struct JsonlScratch {
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen, time;
    std::vector<uint8_t> status, head, bytes;
};
thread_local JsonlScratch tlsScratch;

// the group's head into `head`; false (bounded only): beyond LC_JSONL_MAX_HEAD_BYTES, which the device path does not take
bool groupHead(const PipelineEventGroup& group, std::vector<uint8_t>& head, bool bounded) {
    std::vector<const char*> kp, vp;
    std::vector<uint32_t> kl, vl;
    for (const auto& kv : group.GetTags()) {
        kp.push_back(kv.first.data());
        kl.push_back(uint32_t(kv.first.size()));
        vp.push_back(kv.second.data());
        vl.push_back(uint32_t(kv.second.size()));
    }
    size_t need = 0;
    (void)lc_jsonl_head(kp.data(), kl.data(), vp.data(), vl.data(), uint32_t(kp.size()), nullptr, 0, &need);
    if (bounded && need > LC_JSONL_MAX_HEAD_BYTES) return false;
    head.resize(need);
    return lc_jsonl_head(kp.data(), kl.data(), vp.data(), vl.data(), uint32_t(kp.size()), head.data(), head.size(), &need) == LC_OK;
}

// JsonEventGroupSerializer over the log events of a group as they are; an event that is not a log event is skipped
void writeLogEvents(const PipelineEventGroup& group, std::vector<uint8_t>& bytes) {
    bytes.clear();
    std::vector<uint8_t> head;
    if (!groupHead(group, head, false)) return;
    for (const PipelineEventPtr& e : group.GetEvents()) {
        if (!e.Is<LogEvent>()) continue;
        const LogEvent& ev = e.Cast<LogEvent>();
        if (ev.Empty()) continue;
        bytes.insert(bytes.end(), head.begin(), head.end());
        const std::string t = std::to_string(uint32_t(ev.GetTimestamp()));
        bytes.insert(bytes.end(), t.begin(), t.end());
        for (const auto& kv : ev) {
            bytes.push_back(',');
            bytes.push_back('"');
            lcjsonl::appendEscaped(bytes, reinterpret_cast<const uint8_t*>(kv.first.data()), kv.first.size());
            bytes.push_back('"');
            bytes.push_back(':');
            bytes.push_back('"');
            lcjsonl::appendEscaped(bytes, reinterpret_cast<const uint8_t*>(kv.second.data()), kv.second.size());
            bytes.push_back('"');
        }
        bytes.push_back('}');
        bytes.push_back('\n');
    }
}
}  // namespace

bool ProcessorJsonlGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!mParse.Init(config, error)) return false;
    if (!ParseProbe::serves(mParse)) return true;
    std::vector<std::string> keys;
    std::vector<uint32_t> items[2];
    if (!ParseProbe::itemLists(mParse, keys, items, mFailedTally)) return true;
    std::vector<const char*> keyPtr;
    std::vector<uint32_t> keyLen;
    for (const std::string& k : keys) {
        keyPtr.push_back(k.data());
        keyLen.push_back(uint32_t(k.size()));
    }
    char err[256];
    // (a plan beyond its bounds is refused: the processor then takes its host path for every group)
    if (lc_jsonl_plan_create(keyPtr.data(), keyLen.data(), uint32_t(keys.size()), items[0].data(), uint32_t(items[0].size() / 2), items[1].data(),
                             uint32_t(items[1].size() / 2), &mPlan, err, sizeof err) != LC_OK)
        mPlan = nullptr;
    return true;
}

// the groups ProcessorPipelineGpu::ProcessFused would serve
bool ProcessorJsonlGpu::DevicePathServes(const PipelineEventGroup& group) const {
    if (!mPlan || mParse.AlarmsWanted()) return false;
    for (const PipelineEventPtr& e : group.GetEvents()) {
        if (!e.Is<LogEvent>()) return false;
        const LogEvent& ev = e.Cast<LogEvent>();
        if (ev.Size() != 1 || !ev.HasContent(mParse.mSourceKey)) return false;
    }
    return true;
}

int ProcessorJsonlGpu::SerializeOnDevice(PipelineEventGroup& group, const uint8_t** out, size_t* outLen, bool* undecided) {
    JsonlScratch& S = tlsScratch;
    const EventsContainer& events = group.GetEvents();
    const uint32_t n = uint32_t(events.size());
    S.linePtr.resize(n);
    S.lineLen.resize(n);
    S.time.resize(n);
    S.status.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const LogEvent& ev = events[i].Cast<LogEvent>();
        const StringView raw = ev.GetContent(mParse.mSourceKey);
        S.linePtr[i] = reinterpret_cast<const uint8_t*>(raw.data());
        S.lineLen[i] = uint32_t(raw.size());
        S.time[i] = uint32_t(ev.GetTimestamp());
    }
    const int rc = lc_jsonl_match_encode_host(mPlan, mParse.mReg, S.linePtr.data(), S.lineLen.data(), n, S.time.data(), S.head.data(),
                                              uint32_t(S.head.size()), out, outLen, nullptr, S.status.data());
    if (rc != LC_OK) {
        mParse.ReportDeviceFailure(rc, n);
        mParse.mDeviceFailedEventsTotal += n;
        return rc;
    }
    Tally tally;
    for (uint32_t i = 0; i < n; ++i) {
        if (S.status[i] == LC_MATCH) {
            ++tally.outSuccessful;
            continue;
        }
        if (S.status[i] == LC_OVERFLOW) {  // not decided: neither a success nor a failure -- the chained path books it exactly
            *undecided = true;
            return LC_OK;
        }
        if (S.status[i] == LC_GAVE_UP) ++tally.complexityExceeded;
        tally.outFailed += mFailedTally.outFailed;
        tally.discarded += mFailedTally.discarded;
        tally.outSuccessful += mFailedTally.outSuccessful;
    }
    mParse.AddTally(tally);
    return LC_OK;
}

// the parser's own Process on a copy of the events (views into the same buffers), then the host writer
void ProcessorJsonlGpu::SerializeOnHost(PipelineEventGroup& group, const uint8_t** out, size_t* outLen) {
    PipelineEventGroup copy(std::make_shared<SourceBuffer>());
    for (const auto& kv : group.GetAllMetadata()) copy.SetMetadataNoCopy(kv.first, kv.second);
    for (const auto& kv : group.GetTags()) copy.SetTag(kv.first.to_string(), kv.second.to_string());
    for (const PipelineEventPtr& e : group.GetEvents()) {
        if (e.Is<LogEvent>()) {
            const LogEvent& ev = e.Cast<LogEvent>();
            LogEvent* c = copy.AddLogEvent();
            if (ev.GetTimestampNanosecond()) c->SetTimestamp(ev.GetTimestamp(), *ev.GetTimestampNanosecond());
            else c->SetTimestamp(ev.GetTimestamp());
            for (const auto& kv : ev) c->SetContentNoCopy(kv.first, kv.second);
        } else if (e.Is<RawEvent>()) {
            copy.AddRawEvent()->SetContentNoCopy(e.Cast<RawEvent>().GetContent());
        } else {
            copy.AddMetricEvent();  // (counted by the parser as an event it does not support; never written)
        }
    }
    mParse.Process(copy);
    writeLogEvents(copy, tlsScratch.bytes);
    *out = tlsScratch.bytes.data();
    *outLen = tlsScratch.bytes.size();
}

int ProcessorJsonlGpu::Serialize(PipelineEventGroup& group, const uint8_t** out, size_t* outLen, int* fused) {
    *out = nullptr;
    *outLen = 0;
    *fused = 0;
    if (group.GetEvents().empty()) return LC_OK;
    if (DevicePathServes(group) && groupHead(group, tlsScratch.head, true)) {
        bool undecided = false;
        const int rc = SerializeOnDevice(group, out, outLen, &undecided);
        if (rc != LC_OK) {
            ++mFailedTrips;
            *out = nullptr;
            *outLen = 0;
            return rc;
        }
        if (!undecided) {
            *fused = 1;
            ++mGroupsDevice;
            mBytes += *outLen;
            return LC_OK;
        }
    }
    const uint64_t failedBefore = mParse.mDeviceFailedEventsTotal;
    SerializeOnHost(group, out, outLen);
    if (mParse.mDeviceFailedEventsTotal != failedBefore) {  // the parser's trip failed: its events went on unparsed, nothing to hand out
        ++mFailedTrips;
        *out = nullptr;
        *outLen = 0;
        return LC_ERR_HIP;
    }
    ++mGroupsHost;
    mBytes += *outLen;
    return LC_OK;
}

}  // namespace logtail

struct lc_jsonl_processor {
    logtail::ProcessorJsonlGpu impl;
};

extern "C" int lc_jsonl_processor_create(const char* config_json, lc_jsonl_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_jsonl_processor_destroy(lc_jsonl_processor_t* p) { delete p; }

extern "C" int lc_jsonl_processor_serialize(lc_jsonl_processor_t* p, lc_event_group_t* group, const uint8_t** out, size_t* out_len, int* fused) {
    if (!p || !group || !out || !out_len || !fused) return LC_ERR_ARG;
    logtail::PipelineEventGroup& g = *static_cast<logtail::PipelineEventGroup*>(lc_group_native(group));
    // a group that needs the device must not be half-processed when there is none: check first, fail loudly (lc_processor_process)
    if (!p->impl.mParse.IsWholeLineMode() && lc_device_count() <= 0) {
        for (const auto& e : g.GetEvents())
            if (e.Is<logtail::LogEvent>() && e.Cast<logtail::LogEvent>().HasContent(p->impl.mParse.mSourceKey)) return LC_ERR_NO_DEVICE;
    }
    return p->impl.Serialize(g, out, out_len, fused);
}

extern "C" int lc_jsonl_serialize_group_host(lc_event_group_t* group, const uint8_t** out, size_t* out_len) {
    if (!group || !out || !out_len) return LC_ERR_ARG;
    std::vector<uint8_t>& bytes = logtail::tlsScratch.bytes;
    logtail::writeLogEvents(*static_cast<logtail::PipelineEventGroup*>(lc_group_native(group)), bytes);
    *out = bytes.data();
    *out_len = bytes.size();
    return LC_OK;
}

extern "C" int lc_jsonl_processor_counters(const lc_jsonl_processor_t* p, uint64_t parse[LC_CNT_COUNT], uint64_t own[LC_JSONL_CNT_COUNT]) {
    if (!p || !parse || !own) return LC_ERR_ARG;
    for (int i = 0; i < LC_CNT_COUNT; ++i) parse[i] = 0;
    const logtail::ProcessorParseRegexGpu& parser = p->impl.mParse;
    parse[LC_CNT_DISCARDED_EVENTS] = parser.mDiscardedEventsTotal;
    parse[LC_CNT_OUT_FAILED_EVENTS] = parser.mOutFailedEventsTotal;
    parse[LC_CNT_OUT_KEY_NOT_FOUND] = parser.mOutKeyNotFoundEventsTotal;
    parse[LC_CNT_OUT_SUCCESSFUL_EVENTS] = parser.mOutSuccessfulEventsTotal;
    parse[LC_CNT_COMPLEXITY_EXCEEDED] = parser.mComplexityExceededEventsTotal;
    parse[LC_CNT_UNDECIDED_EVENTS] = parser.mUndecidedEventsTotal;
    parse[LC_CNT_DEVICE_FAILED_EVENTS] = parser.mDeviceFailedEventsTotal;
    own[LC_JSONL_CNT_GROUPS_DEVICE] = p->impl.mGroupsDevice;
    own[LC_JSONL_CNT_GROUPS_HOST] = p->impl.mGroupsHost;
    own[LC_JSONL_CNT_FAILED_TRIPS] = p->impl.mFailedTrips;
    own[LC_JSONL_CNT_BYTES] = p->impl.mBytes;
    return LC_OK;
}
