// tests/native/prom_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_prom_parse_metric_gpu on a box without a GPU.
//
// csrc/processor_parse_prom_gpu.cpp (Init, the gather, the second trip, the event build, counters, alarms) asks the engine for ONE
// thing: lc_prom_parse_host.  This translation unit answers it on the CPU by running the PRODUCT's per-line routine -- promParseLine()
// of csrc/prom_vm.hpp, the function the kernel runs per lane, compiled here for the host -- over a copy of each line that ends exactly
// at the line's end, and then promFinishHost() as the real entry does.  tests/helpers/prom_product.py builds
// processor_parse_prom_gpu.cpp + event_model.cpp + this file into tests/_build/libprom_double.so.  Never linked into
// loongcollector_amd/lib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc_prom.h"
#ifndef LC_PROM_DOUBLE_ROUTINES_ONLY  // (routines only: the mutation builds of tests/test_prom_host.py, this file and prom_vm.hpp alone)
#include "../../loongcollector_amd/csrc/event_model.hpp"
#endif
#include "../../loongcollector_amd/csrc/prom_vm.hpp"

static uint64_t gParseCalls = 0, gParseLines = 0;
static int gFailNext = 0;

namespace {
void store(const PromLine& r, const lc_prom_out_t* out, size_t i) {
    out->status[i] = r.status;
    out->flags[i] = r.flags;
    out->name[i * 2] = r.name.begin, out->name[i * 2 + 1] = r.name.end;
    out->value[i] = r.value;
    out->value_span[i * 2] = r.valueSpan.begin, out->value_span[i * 2 + 1] = r.valueSpan.end;
    out->time_span[i * 2] = r.timeSpan.begin, out->time_span[i * 2 + 1] = r.timeSpan.end;
    out->secs[i] = r.secs;
    out->nanos[i] = r.nanos;
    out->nlabels[i] = r.nlabels;
}
#ifndef LC_PROM_DOUBLE_ROUTINES_ONLY
void put32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
void put64(std::string& o, uint64_t v) { o.append(reinterpret_cast<const char*>(&v), 8); }
void putText(std::string& o, logtail::StringView s) {
    put32(o, uint32_t(s.size()));
    o.append(s.data(), s.size());
}
#endif
}  // namespace

extern "C" {
int lc_device_count(void) { return 1; }
const char* lc_last_error(void) { return "the double's trip was told to fail"; }

// one line through the product's routine, the line placed `head` bytes behind a 16-byte boundary and `tail` arbitrary bytes behind it
// (the routine must not see them).  out: arrays of ONE entry, labels int32[W][4].  finish: promFinishHost behind it.  Returns the
// tokens finished.
uint32_t pd_parse_one(const uint8_t* line, uint32_t len, uint32_t head, const uint8_t* tail, uint32_t tailLen, int honor, uint32_t W,
                      const lc_prom_out_t* out, int finish) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[size_t(len) + tailLen + 1]);
    if (len) std::memcpy(copy.get(), line, len);
    if (tailLen) std::memcpy(copy.get() + len, tail, tailLen);
    PromLine r;
    promParseLineHost(copy.get(), len, honor != 0, out->labels, W, r, head);
    const uint32_t finished = finish ? promFinishHost(copy.get(), r) : 0;
    store(r, out, 0);
    return finished;
}
int lc_prom_parse_host(int honor_timestamps, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const lc_prom_out_t* out, uint32_t W,
                       uint64_t* deferred_tokens) {
    if (deferred_tokens) *deferred_tokens = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !out) return LC_ERR_ARG;
    if (gFailNext) {
        --gFailNext;
        return LC_ERR_HIP;
    }
    ++gParseCalls;
    gParseLines += n;
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the line is an out-of-bounds read of this heap block
        std::unique_ptr<uint8_t[]> copy(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copy.get(), lines[i], len[i]);
        PromLine r;
        promParseLineHost(copy.get(), len[i], honor_timestamps != 0, out->labels + size_t(i) * W * 4, W, r, i & 15u);
        const uint32_t finished = promFinishHost(copy.get(), r);
        if (deferred_tokens) *deferred_tokens += finished;
        store(r, out, i);
    }
    return LC_OK;
}
// the routine alone over lines that lie back to back in ONE resident buffer (line i = data[off[i] .. off[i + 1])): no copy, no
// allocation -- what tools/prom_bench.py times as "the per-line routine on one host thread".  Returns the tokens finished.
uint64_t pd_parse_resident(int honor, const uint8_t* data, const int32_t* off, uint32_t n, const lc_prom_out_t* out, uint32_t W, int finish) {
    uint64_t finished = 0;
    for (uint32_t i = 0; i < n; ++i) {
        PromLine r;
        promParseLineHost(data + off[i], uint32_t(off[i + 1] - off[i]), honor != 0, out->labels + size_t(i) * W * 4, W, r, uint32_t(off[i]) & 15u);
        if (finish) finished += promFinishHost(data + off[i], r);
        store(r, out, i);
    }
    return finished;
}
// promUnescape of line[vb, ve) -> out (at least ve - vb bytes); returns the text's length
uint32_t pd_unescape(const uint8_t* line, int32_t vb, int32_t ve, uint8_t* out) {
    std::string text;
    promUnescape(line, vb, ve, text);
    std::memcpy(out, text.data(), text.size());
    return uint32_t(text.size());
}
void pd_fail_next_trips(int n) { gFailNext = n; }
void pd_parse_stats(uint64_t out[2]) {
    out[0] = gParseCalls;
    out[1] = gParseLines;
}

#ifndef LC_PROM_DOUBLE_ROUTINES_ONLY
// A group of n events -- kind[i] 0: a RawEvent whose content is a copy of lines[i], else a LogEvent -- with the scrape timestamp
// `scrape` (NULL: not set) -> lc_prom_processor_process_native -> the events left, packed (malloc'ed; pd_free):
//   u32 events | per event: type u8, secs i64, nanos u32, has_nanos u8 | metric events: bits u64, name, u32 tags, per tag key, value,
//   u8 the value is a view into a raw event's content (texts: u32 length + bytes)
char* pd_process(lc_prom_processor_t* p, const uint8_t* const* lines, const uint32_t* len, const uint8_t* kind, uint32_t n, const char* scrape, int* rc_out,
                 size_t* out_len) {
    auto sb = std::make_shared<logtail::SourceBuffer>();
    logtail::PipelineEventGroup group(sb);
    if (scrape) group.SetMetadata(logtail::EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC, std::string(scrape));
    std::vector<std::pair<const char*, size_t>> sources;
    for (uint32_t i = 0; i < n; ++i) {
        if (kind[i]) {
            group.AddLogEvent()->SetContent(std::string("content"), std::string(reinterpret_cast<const char*>(lines[i]), len[i]));
            continue;
        }
        const logtail::StringBuffer b = sb->CopyString(reinterpret_cast<const char*>(lines[i]), len[i]);
        group.AddRawEvent()->SetContentNoCopy(logtail::StringView(b.data, b.size));
        sources.emplace_back(b.data, b.size);
    }
    *rc_out = lc_prom_processor_process_native(p, &group);
    std::string o;
    put32(o, uint32_t(group.GetEvents().size()));
    for (const logtail::PipelineEventPtr& e : group.GetEvents()) {
        o.push_back(char(e->GetType()));
        put64(o, uint64_t(int64_t(e->GetTimestamp())));
        put32(o, e->GetTimestampNanosecond() ? *e->GetTimestampNanosecond() : 0);
        o.push_back(e->GetTimestampNanosecond() ? 1 : 0);
        if (!e.Is<logtail::MetricEvent>()) continue;
        const logtail::MetricEvent& m = e.Cast<logtail::MetricEvent>();
        uint64_t bits = 0;
        if (m.Is<logtail::UntypedSingleValue>()) std::memcpy(&bits, &m.GetValue<logtail::UntypedSingleValue>()->mValue, 8);
        put64(o, bits);
        putText(o, m.GetName());
        put32(o, uint32_t(m.TagsSize()));
        for (auto it = m.TagsBegin(); it != m.TagsEnd(); ++it) {
            putText(o, it->first);
            putText(o, it->second);
            bool view = false;
            for (const auto& s : sources) view = view || (it->second.data() >= s.first && it->second.data() + it->second.size() <= s.first + s.second);
            o.push_back(view ? 1 : 0);
        }
    }
    char* out = static_cast<char*>(std::malloc(o.size() ? o.size() : 1));
    std::memcpy(out, o.data(), o.size());
    *out_len = o.size();
    return out;
}
void* lc_group_native(lc_event_group_t*) { return nullptr; }  // (the fixture wrapper of c_processor_slot.cpp is not part of this build)
#endif
void pd_free(void* p) { std::free(p); }
void lc_free(void* p) { std::free(p); }
}  // extern "C"
