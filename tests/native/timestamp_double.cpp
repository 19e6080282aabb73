// tests/native/timestamp_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_parse_timestamp_gpu on a box without a GPU.
//
// csrc/processor_parse_timestamp_gpu.cpp (Init, the gather, the zone, the year modes, the cache walk, counters, alarms) asks the engine
// for ONE thing: lc_strptime_parse_host.  This translation unit answers it on the CPU by running the PRODUCT's per-value routine --
// strptimeRun() of csrc/strptime_vm.hpp, the function strptime_kernel runs per lane, compiled here for the host -- over a copy of each
// value that ends exactly at the value's end (a read behind it is an out-of-bounds read of a heap block of that size).  same_as_prev is
// computed by its definition.  tests/test_timestamp_host.py builds
//   processor_parse_timestamp_gpu.cpp + strptime_program.cpp + event_model.cpp + this file
// into tests/_build/libtimestamp_double.so.  It lives under tests/ and is never linked into loongcollector_amd/lib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc_timestamp.h"
#include "../../loongcollector_amd/csrc/event_model.hpp"
#include "../../loongcollector_amd/csrc/strptime_program.hpp"

struct lc_strptime {
    StrptimeProgram prog;
};
static uint64_t gParseCalls = 0, gParseValues = 0;
// what the processor does behind a failed device trip: td_fail_next_trips(n) fails the next n engine calls, td_fail_after(k) lets
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
const char* lc_last_error(void) { return "the timestamp double has no device"; }
int lc_device_count(void) { return 1; }

int lc_strptime_create(const char* format, lc_strptime_t** out, char* err, size_t errcap) {
    if (!out || !format) return LC_ERR_ARG;
    *out = nullptr;
    StrptimeProgram prog;
    std::string error;
    if (!strptimeCompile(format, &prog, &error)) {
        if (err && errcap) std::snprintf(err, errcap, "%s", error.c_str());
        return LC_ERR_UNSUPPORTED;
    }
    *out = new lc_strptime{prog};
    return LC_OK;
}
void lc_strptime_destroy(lc_strptime_t* t) { delete t; }
uint32_t lc_strptime_program(const lc_strptime_t* t, uint32_t words[LC_TS_MAX_PROGRAM]) {
    if (!t) return 0;
    if (words) std::memcpy(words, t->prog.words, sizeof t->prog.words);
    return t->prog.n;
}

// one value through the product's routine
void td_parse_one(const lc_strptime_t* t, const uint8_t* val, uint32_t len, uint8_t* status, int64_t* secs, uint32_t* nanos, int32_t* matched,
                  int32_t* fracLen) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(copy.get(), val, len);
    const StrptimeResult r = strptimeRun(HostSpanSource{copy.get()}, len, t->prog.words, t->prog.n, kStrptimeNames.b);
    *status = r.status;
    *secs = r.secs;
    *nanos = r.nanos;
    *matched = r.matched;
    *fracLen = r.fracLen;
}
int lc_strptime_parse_host(lc_strptime_t* t, const uint8_t* const* vals, const uint32_t* len, uint32_t n, const lc_ts_out_t* out) {
    if (!t || (n && (!vals || !len || !out))) return LC_ERR_ARG;
    if (tripFails()) return LC_ERR_HIP;
    ++gParseCalls;
    gParseValues += n;
    for (uint32_t i = 0; i < n; ++i) {
        td_parse_one(t, vals[i], len[i], out->status + i, out->secs + i, out->nanos + i, out->matched + i, out->frac_len + i);
        uint8_t same = 0;
        if (i && (out->status[i] & LC_TS_OK) && (out->status[i - 1] & LC_TS_OK)) {
            const int32_t a = out->matched[i] - out->frac_len[i], b = out->matched[i - 1] - out->frac_len[i - 1];
            same = a == b && std::memcmp(vals[i], vals[i - 1], size_t(a)) == 0;
        }
        out->same_as_prev[i] = same;
    }
    return LC_OK;
}
void td_fail_next_trips(int n) { gFailNext = n; }
void td_fail_after(int k) { gFailAfter = k; }
void td_parse_stats(uint64_t out[2]) {
    out[0] = gParseCalls;
    out[1] = gParseValues;
}

// fixture JSON in -> lc_timestamp_processor_process_native -> fixture JSON out (malloc'ed; td_free).  rc_out: the processor's return code
char* td_process_json_rc(lc_timestamp_processor_t* p, const char* groupJson, int* rc_out, char* err, size_t errcap) {
    logtail::PipelineEventGroup group(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!group.FromJsonString(groupJson, &error)) {
        std::snprintf(err, errcap, "%s", error.c_str());
        return nullptr;
    }
    *rc_out = lc_timestamp_processor_process_native(p, &group);
    return strdup(group.ToJsonString().c_str());
}
// the same; a failed trip answers nullptr
char* td_process_json(lc_timestamp_processor_t* p, const char* groupJson, char* err, size_t errcap) {
    int rc = LC_OK;
    char* out = td_process_json_rc(p, groupJson, &rc, err, errcap);
    if (out && rc != LC_OK) {
        std::snprintf(err, errcap, "lc_timestamp_processor_process_native failed: %d", rc);
        std::free(out);
        return nullptr;
    }
    return out;
}
void* lc_group_native(lc_event_group_t*) { return nullptr; }  // (the fixture wrapper of c_processor_slot.cpp is not part of this build)
void td_free(void* p) { std::free(p); }
void lc_free(void* p) { std::free(p); }
}  // extern "C"
