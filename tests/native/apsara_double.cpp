// tests/native/apsara_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_parse_apsara_gpu on a box without a GPU.
//
// csrc/processor_parse_apsara_gpu.cpp (Init, the gather, the zone, the cache replay, the second trip, the stitch, counters, alarms) asks
// the engine for ONE thing: lc_apsara_parse_host.  This translation unit answers it on the CPU by running the PRODUCT's per-line
// routine -- apsaraParseLine() of csrc/apsara_vm.hpp, the function apsara_parse_kernel runs per lane, compiled here for the host -- over
// a copy of each line that ends exactly at the line's end, through a source that answers junk for every byte outside the line.
// tests/helpers/apsara_double.py builds processor_parse_apsara_gpu.cpp + processor_parse_timestamp_gpu.cpp (lc_timestamp_zone_seconds)
// + strptime_program.cpp + processor_parse_regex_gpu.cpp (GpuCommonParserOptions) + event_model.cpp + this file into tests/_build/libapsara_double.so.  Never linked into loongcollector_amd/lib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc_apsara.h"
#include "../../loongcollector_amd/csrc/apsara_vm.hpp"
#include "../../loongcollector_amd/csrc/event_model.hpp"

static uint64_t gParseCalls = 0, gParseLines = 0;
static int gFailNext = 0;

extern "C" {
const char* lc_last_error(void) { return "the Apsara double has no device"; }
int lc_device_count(void) { return 1; }
// (processor_parse_timestamp_gpu.cpp is linked for lc_timestamp_zone_seconds; its engine is not part of this build)
int lc_strptime_create(const char*, lc_strptime_t** out, char*, size_t) {
    if (out) *out = nullptr;
    return LC_ERR_UNSUPPORTED;
}
void lc_strptime_destroy(lc_strptime_t*) {}
int lc_strptime_parse_host(lc_strptime_t*, const uint8_t* const*, const uint32_t*, uint32_t, const lc_ts_out_t*) { return LC_ERR_UNSUPPORTED; }
// (processor_parse_regex_gpu.cpp is linked for GpuCommonParserOptions; nothing here builds a regex processor)
int lc_regex_compile(const char*, size_t, uint32_t, int, lc_regex_t** out, char*, size_t) {
    if (out) *out = nullptr;
    return LC_ERR_NO_DEVICE;
}
void lc_regex_free(lc_regex_t*) {}
int lc_regex_mark_count(const lc_regex_t*) { return 0; }
int lc_regex_match_host_views(lc_regex_t*, const uint8_t* const*, const uint32_t*, uint32_t, uint32_t, int32_t*, uint8_t*) { return LC_ERR_NO_DEVICE; }

// one line through the product's routine, the line placed `head` bytes behind a 16-byte boundary and `tail` arbitrary bytes behind it
// (the routine must not see them).  pairs: room for W triples
void ad_parse_one(const uint8_t* line, uint32_t len, uint32_t W, uint32_t head, const uint8_t* tail, uint32_t tailLen, uint8_t* status,
                  int64_t* secs, uint32_t* nanos, int32_t* base, uint32_t* npairs, int32_t* pairs) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[size_t(len) + tailLen + 1]);
    if (len) std::memcpy(copy.get(), line, len);
    if (tailLen) std::memcpy(copy.get() + len, tail, tailLen);
    ApsaraLine r;
    apsaraParseHost(copy.get(), len, W, reinterpret_cast<ApsaraPair*>(pairs), r, head);
    *status = r.status;
    *secs = r.secs;
    *nanos = r.nanos;
    std::memcpy(base, r.base, sizeof r.base);
    *npairs = r.npairs;
}
int lc_apsara_parse_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, const lc_apsara_out_t* out) {
    if (n && (!lines || !len || !out)) return LC_ERR_ARG;
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
        ApsaraLine r;
        apsaraParseHost(copy.get(), len[i], W, reinterpret_cast<ApsaraPair*>(out->pairs) + size_t(i) * W, r, i & 15u);
        out->status[i] = r.status;
        out->secs[i] = r.secs;
        out->nanos[i] = r.nanos;
        std::memcpy(out->base + size_t(i) * 8, r.base, sizeof r.base);
        out->npairs[i] = r.npairs;
    }
    return LC_OK;
}
// the routine alone over lines that lie back to back in ONE resident buffer (line i = data[off[i] .. off[i + 1])): no copy, no
// allocation -- what tools/apsara_bench.py times as "the host routine on one thread"
void ad_parse_resident(const uint8_t* data, const int32_t* off, uint32_t n, uint32_t W, const lc_apsara_out_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        ApsaraLine r;
        apsaraParseHost(data + off[i], uint32_t(off[i + 1] - off[i]), W, reinterpret_cast<ApsaraPair*>(out->pairs) + size_t(i) * W, r, uint32_t(off[i]) & 15u);
        out->status[i] = r.status;
        out->secs[i] = r.secs;
        out->nanos[i] = r.nanos;
        std::memcpy(out->base + size_t(i) * 8, r.base, sizeof r.base);
        out->npairs[i] = r.npairs;
    }
}
void ad_fail_next_trips(int n) { gFailNext = n; }
void ad_parse_stats(uint64_t out[2]) {
    out[0] = gParseCalls;
    out[1] = gParseLines;
}

// fixture JSON in -> lc_apsara_processor_process_native -> fixture JSON out (malloc'ed; ad_free).  rc_out: the processor's return code
char* ad_process_json_rc(lc_apsara_processor_t* p, const char* groupJson, int* rc_out, char* err, size_t errcap) {
    logtail::PipelineEventGroup group(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!group.FromJsonString(groupJson, &error)) {
        std::snprintf(err, errcap, "%s", error.c_str());
        return nullptr;
    }
    *rc_out = lc_apsara_processor_process_native(p, &group);
    return strdup(group.ToJsonString().c_str());
}
void* lc_group_native(lc_event_group_t*) { return nullptr; }  // (the fixture wrapper of c_processor_slot.cpp is not part of this build)
void ad_free(void* p) { std::free(p); }
void lc_free(void* p) { std::free(p); }
}  // extern "C"
