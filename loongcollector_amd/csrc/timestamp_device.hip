// timestamp_device.hip -- the engine level of the timestamp parser (include/lc_timestamp.h): the handle, the launch of strptime_kernel
// (strptime_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/lc_timestamp.h"
#include "runtime_internal.hpp"
#include "strptime_kernel.hpp"
#include "strptime_program.hpp"
#include "trip_buffers.hpp"

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
struct TimestampThread : TripThread<TimestampThread> {
    TripBuf hIn, hOut, dIn, dOut;
    TimestampThread() : TripThread(true) { hIn.pinned = hOut.pinned = true; }
    ~TimestampThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dOut}); }
};
thread_local TimestampThread tlsTimestamp;

constexpr size_t kChunkBytes = 32u << 20;   // value bytes per trip
constexpr uint32_t kChunkValues = 1u << 20;  // and at most this many values
}  // namespace

void lcTimestampThreadRelease() { tlsTimestamp.release(); }

extern "C" int lc_strptime_parse_host(lc_strptime_t* t, const uint8_t* const* vals, const uint32_t* len, uint32_t n, const lc_ts_out_t* out) {
    if (!t) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!vals || !len || !outComplete(out)) return LC_ERR_ARG;
    TimestampThread& T = tlsTimestamp;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the timestamp parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    uint32_t next = 0;
    while (next < n) {
        // a chunk up: the values back to back, then (64-byte aligned) their offsets and (begin, end) pairs -- ONE copy; down: the six
        // result arrays in one block -- ONE copy.  same_as_prev of a chunk's first value is computed against nothing: the chunk starts
        // one value early instead (the value before is parsed again and its results are dropped).
        const uint32_t lead = next ? 1u : 0u;
        const uint32_t first = next - lead;
        uint32_t cnt = lead;
        size_t bytes = lead ? len[first] : 0;
        if (!tripCarve(len, next, n, kChunkValues, kChunkBytes, 0, 0, &cnt, &bytes)) {
            lcSetLastError("lc_strptime_parse_host: a value of 2 GiB or more");
            return LC_ERR_ARG;
        }
        const size_t offAt = tripOffAt(bytes);
        const size_t spanAt = offAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t inBytes = spanAt + size_t(cnt) * 8;
        const size_t nanosAt = tripRoundUp(size_t(cnt) * 8, 64);
        const size_t matchedAt = nanosAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t fracAt = matchedAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t statusAt = fracAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t sameAt = statusAt + tripRoundUp(cnt, 64);
        const size_t outBytes = sameAt + tripRoundUp(cnt, 64);
        LC_HIP_TRY(T.hIn.ensure(inBytes));
        LC_HIP_TRY(T.dIn.ensure(inBytes));
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
        tripPackLines(hIn, offAt, vals, len, first, cnt);
        int32_t* hSpan = reinterpret_cast<int32_t*>(hIn + spanAt);
        for (uint32_t i = 0; i < cnt; ++i) {
            hSpan[2 * i] = 0;
            hSpan[2 * i + 1] = int32_t(len[first + i]);
        }
        uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
        uint8_t* dOut = static_cast<uint8_t*>(T.dOut.p);
        LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
        const lc_ts_out_t dev_out{dOut + statusAt, reinterpret_cast<int64_t*>(dOut), reinterpret_cast<uint32_t*>(dOut + nanosAt),
                                  reinterpret_cast<int32_t*>(dOut + matchedAt), reinterpret_cast<int32_t*>(dOut + fracAt), dOut + sameAt};
        const lcts::Values v{dIn, reinterpret_cast<const uint32_t*>(dIn + offAt), reinterpret_cast<const int32_t*>(dIn + spanAt), 2, 0, nullptr, 0};
        int rc = launchParse(t, v, cnt, &dev_out, T.stream);
        if (rc == LC_OK) {
            const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(timestamp results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint8_t* hOut = static_cast<const uint8_t*>(T.hOut.p);
        const uint32_t got = cnt - lead;
        std::memcpy(out->secs + next, hOut + size_t(lead) * 8, size_t(got) * 8);
        std::memcpy(out->nanos + next, hOut + nanosAt + size_t(lead) * 4, size_t(got) * 4);
        std::memcpy(out->matched + next, hOut + matchedAt + size_t(lead) * 4, size_t(got) * 4);
        std::memcpy(out->frac_len + next, hOut + fracAt + size_t(lead) * 4, size_t(got) * 4);
        std::memcpy(out->status + next, hOut + statusAt + lead, got);
        std::memcpy(out->same_as_prev + next, hOut + sameAt + lead, got);
        next += got;
    }
    return LC_OK;
}
