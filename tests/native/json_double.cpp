// tests/native/json_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_parse_json_gpu on a box without a GPU.
//
// csrc/processor_parse_json_gpu.cpp (Init, the gather, the mop-up rule, the stitch, the source-key rules, counters, alarms) asks the
// engine for ONE thing: lc_json_walk_host.  This translation unit answers it on the CPU by running the PRODUCT's per-line routine --
// jsonWalkLine() of csrc/json_vm.hpp, the function json_walk_kernel runs per lane, compiled here for the host -- through JsonHostSource.
// tests/test_json_host.py builds
//   processor_parse_json_gpu.cpp + processor_parse_regex_gpu.cpp (CommonParserOptions) + event_model.cpp + json_host_check.cpp + this
// into tests/_build/libjson_double.so.  It lives under tests/ and is never linked into loongcollector_amd/lib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/lc_json.h"
#include "../../loongcollector_amd/csrc/event_model.hpp"
#include "../../loongcollector_amd/csrc/json_vm.hpp"

static uint64_t gWalkCalls = 0, gWalkLines = 0;
// what the processor does behind a failed device trip: jd_fail_next_trips(n) fails the next n engine calls, jd_fail_after(k) lets
// k calls through and fails the one behind them (the mop-up alone, for k = 1)
static int gFailNext = 0, gFailAfter = -1;
static bool tripFails() {
    if (gFailNext) {
        --gFailNext;
        return true;
    }
    return gFailAfter >= 0 && gFailAfter-- == 0;
}

extern "C" {
const char* lc_last_error(void) { return "the JSON double has no device"; }
int lc_device_count(void) { return 1; }
// (processor_parse_regex_gpu.cpp comes along for GpuCommonParserOptions; its regex processor is never created here)
int lc_regex_compile(const char*, size_t, uint32_t, int, lc_regex_t** out, char*, size_t) {
    if (out) *out = nullptr;
    return LC_ERR_UNSUPPORTED;
}
void lc_regex_free(lc_regex_t*) {}
int lc_regex_mark_count(const lc_regex_t*) { return 0; }
int lc_regex_match_host_views(lc_regex_t*, const uint8_t* const*, const uint32_t*, uint32_t, uint32_t, int32_t*, uint8_t*) { return LC_ERR_NO_DEVICE; }

int lc_json_walk_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* nmembers,
                      uint32_t* errpos, lc_json_member_t* records, uint8_t* shadow, uint64_t* shadow_bytes_moved) {
    if (shadow_bytes_moved) *shadow_bytes_moved = 0;
    if (n && (!lines || !len || !status || !nmembers || !errpos || !shadow || (W && !records))) return LC_ERR_ARG;
    if (tripFails()) return LC_ERR_HIP;
    ++gWalkCalls;
    gWalkLines += n;
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        jsonWalkLineHost(lines[i], len[i], i * 7u, W, records + size_t(i) * W, shadow + at, status + i, nmembers + i, errpos + i);
        at += len[i];
    }
    return LC_OK;
}
void jd_walk_stats(uint64_t out[2]) {
    out[0] = gWalkCalls;
    out[1] = gWalkLines;
}
void jd_fail_next_trips(int n) { gFailNext = n; }
void jd_fail_after(int k) { gFailAfter = k; }

// fixture JSON in -> lc_json_processor_process_native -> fixture JSON out (malloc'ed; jd_free).  rc_out: the processor's return code
char* jd_process_json(lc_json_processor_t* p, const char* groupJson, int* rc_out, char* err, size_t errcap) {
    logtail::PipelineEventGroup group(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!group.FromJsonString(groupJson, &error)) {
        std::snprintf(err, errcap, "%s", error.c_str());
        return nullptr;
    }
    const int rc = lc_json_processor_process_native(p, &group);
    if (rc_out) *rc_out = rc;
    return strdup(group.ToJsonString().c_str());
}
void* lc_group_native(lc_event_group_t*) { return nullptr; }  // (the fixture wrapper of c_processor_slot.cpp is not part of this build)
void jd_free(void* p) { std::free(p); }
void lc_free(void* p) { std::free(p); }
}  // extern "C"
