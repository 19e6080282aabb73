// processor_sls_gpu.cpp -- the processor level of the SLS encoder (include/sls/lc_sls.h): processor_parse_regex_native followed by
// SLSEventGroupSerializer, as one call that leaves the group alone.  The parser is ProcessorParseRegexGpu itself; what an event
// becomes on the wire is READ OFF that class: one probe event with recognisable spans goes through StitchMatched + FinishEvent, one
// through FinishEvent alone for a failed line (as ProcessorPipelineGpu::ProcessFused does for its failed tally), and the contents that
// are left, in their order, are the plan's two item lists.  KeepingSourceWhenParseFail / Succeed, RenamedSourceKey, the legacy raw-log
// copy and the slot order (DelContent leaves a hole, SetContentNoCopy appends, LogEvent.cpp:83-106) cannot drift from the parser's code.
// No HIP here: the tests build this file on a host double of lc_sls_match_encode_host.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sls/lc_sls.h"
#include "parse_processor_shell.hpp"
#include "sls_vm.hpp"

namespace logtail {

class ProcessorSlsGpu {
public:
    ~ProcessorSlsGpu() { lc_sls_plan_free(mPlan); }
    bool Init(const lcjson::Value& config, std::string& error);
    int Serialize(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen, int* fused);

    ProcessorParseRegexGpu mParse;
    std::atomic<uint64_t> mGroupsDevice{0}, mGroupsHost{0}, mFailedTrips{0}, mBytes{0};

private:
    using Tally = ProcessorParseRegexGpu::Tally;
    bool DevicePathServes(const PipelineEventGroup& group) const;
    int SerializeOnDevice(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen, bool* undecided);
    void SerializeOnHost(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen);

    lc_sls_plan_t* mPlan = nullptr;  // null: no device path for this configuration
    Tally mFailedTally;              // what FinishEvent books for ONE line the parser did not match
};

namespace {
// one runner thread's scratch: the gather of the device path, the bytes of the host path
struct SlsScratch {
    std::vector<const uint8_t*> linePtr;
    std::vector<uint32_t> lineLen, time;
    std::vector<int32_t> timeNs;
    std::vector<uint8_t> status, bytes;
};
thread_local SlsScratch tlsScratch;

void putVarint(std::vector<uint8_t>& out, uint32_t v) {
    while (v >= 0x80u) {
        out.push_back(uint8_t(v | 0x80u));
        v >>= 7;
    }
    out.push_back(uint8_t(v));
}
size_t stringSize(size_t n) { return 1 + lcsls::varintSize(uint32_t(n)) + n; }

// the two passes of SLSEventGroupSerializer over the log events of a group as they are (CalculateLogEventSize + SerializeLogEvent)
void writeLogEvents(const PipelineEventGroup& group, bool enableNs, std::vector<uint8_t>& bytes) {
    bytes.clear();
    for (const PipelineEventPtr& e : group.GetEvents()) {
        if (!e.Is<LogEvent>()) continue;
        const LogEvent& ev = e.Cast<LogEvent>();
        if (ev.Empty()) continue;
        const bool ns = enableNs && ev.GetTimestampNanosecond();
        size_t logSZ = 6 + (ns ? 5 : 0);
        for (const auto& kv : ev) {
            const size_t inner = stringSize(kv.first.size()) + stringSize(kv.second.size());
            logSZ += 1 + lcsls::varintSize(uint32_t(inner)) + inner;
        }
        bytes.push_back(0x0A);
        putVarint(bytes, uint32_t(logSZ));
        bytes.push_back(0x08);
        const uint32_t t = uint32_t(ev.GetTimestamp());
        putVarint(bytes, t < lcsls::kMinLogTime ? lcsls::kMinLogTime : t);
        for (const auto& kv : ev) {
            bytes.push_back(0x12);
            putVarint(bytes, uint32_t(stringSize(kv.first.size()) + stringSize(kv.second.size())));
            bytes.push_back(0x0A);
            putVarint(bytes, uint32_t(kv.first.size()));
            bytes.insert(bytes.end(), kv.first.begin(), kv.first.end());
            bytes.push_back(0x12);
            putVarint(bytes, uint32_t(kv.second.size()));
            bytes.insert(bytes.end(), kv.second.begin(), kv.second.end());
        }
        if (ns) {
            bytes.push_back(0x25);
            const uint32_t v = *ev.GetTimestampNanosecond();
            for (int j = 0; j < 4; ++j) bytes.push_back(uint8_t(v >> (8 * j)));
        }
    }
}
}  // namespace

bool ProcessorSlsGpu::Init(const lcjson::Value& config, std::string& error) {
    if (!mParse.Init(config, error)) return false;
    if (mParse.mIsWholeLineMode || !mParse.mKeysDistinct || size_t(mParse.mMarkCount) + 1 <= mParse.mKeys.size()) return true;
    // ---- the probes: a line of L bytes in which group g is the one byte at 2g + 1
    const uint32_t G = uint32_t(mParse.mMarkCount), L = 2 * G + 4;
    PipelineEventGroup probeGroup(std::make_shared<SourceBuffer>());
    const StringBuffer lineBuf = probeGroup.GetSourceBuffer()->AllocateStringBuffer(L);
    std::memset(lineBuf.data, 'x', L);
    const StringView raw(lineBuf.data, L);
    std::vector<int32_t> caps(2 * size_t(G));
    for (uint32_t g = 0; g < G; ++g) {
        caps[2 * g] = int32_t(2 * g + 1);
        caps[2 * g + 1] = int32_t(2 * g + 2);
    }
    std::vector<std::string> keys;
    std::vector<uint32_t> items[2];
    bool readable = true;
    const auto readBack = [&](const LogEvent& ev, std::vector<uint32_t>& list) {
        for (const auto& kv : ev) {
            const size_t at = size_t(reinterpret_cast<uintptr_t>(kv.second.data()) - reinterpret_cast<uintptr_t>(raw.data()));
            uint32_t source = 0;
            if (kv.second.size() == 1 && at >= 1 && at < L && (at & 1u) && (at - 1) / 2 < G) source = uint32_t((at - 1) / 2) + 1;
            else if (!(at == 0 && kv.second.size() == L)) readable = false;  // a value that is neither the line nor a group
            list.push_back(uint32_t(keys.size()));
            list.push_back(source);
            keys.push_back(kv.first.to_string());
        }
    };
    const GroupMetadata& metadata = probeGroup.GetAllMetadata();
    {
        LogEvent* ev = probeGroup.AddLogEvent();
        ev->SetContentNoCopy(StringView(mParse.mSourceKey), raw);
        mParse.StitchMatched(*ev, raw, caps.data());
        Tally tally;
        if (mParse.FinishEvent(*ev, raw, true, metadata, tally)) readBack(*ev, items[0]);
    }
    {
        LogEvent* ev = probeGroup.AddLogEvent();
        ev->SetContentNoCopy(StringView(mParse.mSourceKey), raw);
        mFailedTally = Tally();
        mFailedTally.outFailed = 1;
        if (mParse.FinishEvent(*ev, raw, false, metadata, mFailedTally)) readBack(*ev, items[1]);
    }
    if (!readable) return true;
    std::vector<const char*> keyPtr;
    std::vector<uint32_t> keyLen;
    for (const std::string& k : keys) {
        keyPtr.push_back(k.data());
        keyLen.push_back(uint32_t(k.size()));
    }
    char err[256];
    // (a plan beyond its bounds is refused: the processor then takes its host path for every group)
    if (lc_sls_plan_create(keyPtr.data(), keyLen.data(), uint32_t(keys.size()), items[0].data(), uint32_t(items[0].size() / 2), items[1].data(),
                           uint32_t(items[1].size() / 2), &mPlan, err, sizeof err) != LC_OK)
        mPlan = nullptr;
    return true;
}

// the groups ProcessorPipelineGpu::ProcessFused would serve
bool ProcessorSlsGpu::DevicePathServes(const PipelineEventGroup& group) const {
    if (!mPlan || mParse.AlarmsWanted()) return false;
    for (const PipelineEventPtr& e : group.GetEvents()) {
        if (!e.Is<LogEvent>()) return false;
        const LogEvent& ev = e.Cast<LogEvent>();
        if (ev.Size() != 1 || !ev.HasContent(mParse.mSourceKey)) return false;
        if (ev.GetTimestampNanosecond() && *ev.GetTimestampNanosecond() > 0x7FFFFFFFu) return false;
    }
    return true;
}

int ProcessorSlsGpu::SerializeOnDevice(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen, bool* undecided) {
    SlsScratch& S = tlsScratch;
    const EventsContainer& events = group.GetEvents();
    const uint32_t n = uint32_t(events.size());
    S.linePtr.resize(n);
    S.lineLen.resize(n);
    S.time.resize(n);
    S.timeNs.resize(n);
    S.status.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const LogEvent& ev = events[i].Cast<LogEvent>();
        const StringView raw = ev.GetContent(mParse.mSourceKey);
        S.linePtr[i] = reinterpret_cast<const uint8_t*>(raw.data());
        S.lineLen[i] = uint32_t(raw.size());
        S.time[i] = uint32_t(ev.GetTimestamp());
        S.timeNs[i] = ev.GetTimestampNanosecond() ? int32_t(*ev.GetTimestampNanosecond()) : -1;
    }
    const int rc = lc_sls_match_encode_host(mPlan, mParse.mReg, S.linePtr.data(), S.lineLen.data(), n, S.time.data(), S.timeNs.data(), enableNs ? 1 : 0,
                                            out, outLen, nullptr, S.status.data());
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

// the parser's own Process on a copy of the events (views into the same buffers), then the two passes of SLSEventGroupSerializer
void ProcessorSlsGpu::SerializeOnHost(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen) {
    PipelineEventGroup copy(std::make_shared<SourceBuffer>());
    for (const auto& kv : group.GetAllMetadata()) copy.SetMetadataNoCopy(kv.first, kv.second);
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
    writeLogEvents(copy, enableNs, tlsScratch.bytes);
    *out = tlsScratch.bytes.data();
    *outLen = tlsScratch.bytes.size();
}

int ProcessorSlsGpu::Serialize(PipelineEventGroup& group, bool enableNs, const uint8_t** out, size_t* outLen, int* fused) {
    *out = nullptr;
    *outLen = 0;
    *fused = 0;
    if (group.GetEvents().empty()) return LC_OK;
    if (DevicePathServes(group)) {
        bool undecided = false;
        const int rc = SerializeOnDevice(group, enableNs, out, outLen, &undecided);
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
    SerializeOnHost(group, enableNs, out, outLen);
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

struct lc_sls_processor {
    logtail::ProcessorSlsGpu impl;
};

extern "C" int lc_sls_processor_create(const char* config_json, lc_sls_processor_t** out, char* err, size_t errcap) {
    return logtail::createHandle(config_json, out, err, errcap);
}
extern "C" void lc_sls_processor_destroy(lc_sls_processor_t* p) { delete p; }

extern "C" int lc_sls_processor_serialize(lc_sls_processor_t* p, lc_event_group_t* group, int enable_ns, const uint8_t** out, size_t* out_len,
                                          int* fused) {
    if (!p || !group || !out || !out_len || !fused) return LC_ERR_ARG;
    logtail::PipelineEventGroup& g = *static_cast<logtail::PipelineEventGroup*>(lc_group_native(group));
    // a group that needs the device must not be half-processed when there is none: check first, fail loudly (lc_processor_process)
    if (!p->impl.mParse.IsWholeLineMode() && lc_device_count() <= 0) {
        for (const auto& e : g.GetEvents())
            if (e.Is<logtail::LogEvent>() && e.Cast<logtail::LogEvent>().HasContent(p->impl.mParse.mSourceKey)) return LC_ERR_NO_DEVICE;
    }
    return p->impl.Serialize(g, enable_ns != 0, out, out_len, fused);
}

extern "C" int lc_sls_serialize_group_host(lc_event_group_t* group, int enable_ns, const uint8_t** out, size_t* out_len) {
    if (!group || !out || !out_len) return LC_ERR_ARG;
    std::vector<uint8_t>& bytes = logtail::tlsScratch.bytes;
    logtail::writeLogEvents(*static_cast<logtail::PipelineEventGroup*>(lc_group_native(group)), enable_ns != 0, bytes);
    *out = bytes.data();
    *out_len = bytes.size();
    return LC_OK;
}

extern "C" int lc_sls_processor_counters(const lc_sls_processor_t* p, uint64_t parse[LC_CNT_COUNT], uint64_t own[LC_SLS_CNT_COUNT]) {
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
    own[LC_SLS_CNT_GROUPS_DEVICE] = p->impl.mGroupsDevice;
    own[LC_SLS_CNT_GROUPS_HOST] = p->impl.mGroupsHost;
    own[LC_SLS_CNT_FAILED_TRIPS] = p->impl.mFailedTrips;
    own[LC_SLS_CNT_BYTES] = p->impl.mBytes;
    return LC_OK;
}
