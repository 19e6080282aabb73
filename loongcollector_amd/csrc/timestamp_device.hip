// timestamp_device.hip -- the engine level of the timestamp parser (include/lc_timestamp.h): the handle, the launch of strptime_kernel
// (strptime_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/lc_timestamp.h"
#include "packed_trip.hpp"
#include "strptime_kernel.hpp"
#include "strptime_program.hpp"

struct lc_strptime {
    StrptimeProgram prog;
};

extern "C" int lc_strptime_create(const char* format, lc_strptime_t** out, char* err, size_t errcap) {
    if (!out || !format) return LC_ERR_ARG;
    *out = nullptr;
    StrptimeProgram prog;
    std::string error;
    if (!strptimeCompile(format, &prog, &error)) {
        if (err && errcap) std::snprintf(err, errcap, "%s", error.c_str());
        return LC_ERR_UNSUPPORTED;
    }
    if (err && errcap) err[0] = '\0';
    *out = new lc_strptime{prog};
    return LC_OK;
}
extern "C" void lc_strptime_destroy(lc_strptime_t* t) { delete t; }
extern "C" uint32_t lc_strptime_program(const lc_strptime_t* t, uint32_t words[LC_TS_MAX_PROGRAM]) {
    if (!t) return 0;
    if (words) std::memcpy(words, t->prog.words, sizeof t->prog.words);
    return t->prog.n;
}

static_assert(LC_TS_MAX_PROGRAM == kStrptimeMaxOps, "lc_timestamp.h and strptime_vm.hpp disagree about the program window");

static int launchParse(const lc_strptime* t, const lcts::Values& v, uint32_t n, const lc_ts_out_t* o, hipStream_t st) {
    const dim3 grid((n + lcts::kNewPerBlock - 1) / lcts::kNewPerBlock), block(lcts::kBlock);
    const lcts::Outputs out{o->status, o->secs, o->nanos, o->matched, o->frac_len, o->same_as_prev};
    lcNoteKernel("strptime_kernel");
    hipLaunchKernelGGL(lcts::strptime_kernel, grid, block, 0, st, t->prog, v, n, out);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

static bool outComplete(const lc_ts_out_t* o) {
    return o && o->status && o->secs && o->nanos && o->matched && o->frac_len && o->same_as_prev;
}

static int deviceEntry(lc_strptime_t* t, const lcts::Values& v, uint32_t n, const lc_ts_out_t* d_out, void* stream) {
    if (!t) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!v.data || !v.off || !v.spans || !outComplete(d_out)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the timestamp parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(v.data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchParse(t, v, n, d_out, static_cast<hipStream_t>(stream));
}

extern "C" int lc_strptime_parse_spans_device(lc_strptime_t* t, const uint8_t* d_data, const uint32_t* d_off, const int32_t* d_spans,
                                              uint32_t n, const lc_ts_out_t* d_out, void* stream) {
    return deviceEntry(t, lcts::Values{d_data, d_off, d_spans, 2, 0, nullptr, 0}, n, d_out, stream);
}
extern "C" int lc_strptime_parse_captures_device(lc_strptime_t* t, const uint8_t* d_data, const uint32_t* d_off, const int32_t* d_caps,
                                                 uint32_t ngroups, uint32_t group, const uint8_t* d_line_status, uint32_t match_value,
                                                 uint32_t n, const lc_ts_out_t* d_out, void* stream) {
    if (group >= ngroups) return LC_ERR_ARG;
    return deviceEntry(t, lcts::Values{d_data, d_off, d_caps, 2 * ngroups, 2 * group, d_line_status, match_value}, n, d_out, stream);
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
thread_local PackedThread<struct TimestampTag> tlsTimestamp;
}  // namespace

void lcTimestampThreadRelease() { tlsTimestamp.release(); }

extern "C" int lc_strptime_parse_host(lc_strptime_t* t, const uint8_t* const* vals, const uint32_t* len, uint32_t n, const lc_ts_out_t* out) {
    if (!t) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!vals || !len || !outComplete(out)) return LC_ERR_ARG;
    auto& T = tlsTimestamp;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the timestamp parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    // a chunk: 32 MiB of value bytes, 2^20 values, no cap on the results; up go the values, their offsets and (begin, end) pairs, down
    // come the six result arrays.  same_as_prev of a chunk's first value is computed against nothing: the chunk starts one value early
    // instead (leadIn: the value before is parsed again and its results are dropped).
    PackedTripSpec spec{"lc_strptime_parse_host", "value", 1u << 20, 32u << 20, 0, 0, "hipMemcpyAsync(timestamp results)"};
    spec.leadIn = spec.pairs = true;
    enum { kSecs, kNanos, kMatched, kFrac, kStatus, kSame };
    return packedTrip(
        T, spec, vals, len, n, {8, 4, 4, 4, 1, 1},
        [&](const PackedChunk& c) {
            const lc_ts_out_t dev_out{c.dResult<uint8_t>(kStatus),  c.dResult<int64_t>(kSecs), c.dResult<uint32_t>(kNanos),
                                      c.dResult<int32_t>(kMatched), c.dResult<int32_t>(kFrac), c.dResult<uint8_t>(kSame)};
            const lcts::Values v{c.dIn, reinterpret_cast<const uint32_t*>(c.dIn + c.in.offAt), reinterpret_cast<const int32_t*>(c.dIn + c.in.pairAt),
                                 2, 0, nullptr, 0};
            return launchParse(t, v, c.cnt, &dev_out, T.stream);
        },
        [&](PackedChunk& c) {
            std::memcpy(out->secs + c.next, c.hResult(kSecs, 8), size_t(c.got()) * 8);
            std::memcpy(out->nanos + c.next, c.hResult(kNanos, 4), size_t(c.got()) * 4);
            std::memcpy(out->matched + c.next, c.hResult(kMatched, 4), size_t(c.got()) * 4);
            std::memcpy(out->frac_len + c.next, c.hResult(kFrac, 4), size_t(c.got()) * 4);
            std::memcpy(out->status + c.next, c.hResult(kStatus, 1), c.got());
            std::memcpy(out->same_as_prev + c.next, c.hResult(kSame, 1), c.got());
            return LC_OK;
        });
}
