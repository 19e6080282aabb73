// clog_device.hip -- the engine level of the container stdout parser (include/lc_container_log.h): the launches of
// clog_containerd_kernel / clog_docker_kernel (clog_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/lc_container_log.h"
#include "clog_kernel.hpp"
#include "packed_trip.hpp"

static int launchParse(int format, const uint8_t* d_data, const int32_t* d_off, uint32_t n, const lc_clog_out_t& o, uint8_t* d_shadow,
                       hipStream_t st) {
    const dim3 grid((n + lcclog::kBlock - 1) / lcclog::kBlock), block(lcclog::kBlock);
    if (format == LC_CLOG_CONTAINERD) {
        lcNoteKernel("clog_containerd_kernel");
        hipLaunchKernelGGL(lcclog::clog_containerd_kernel, grid, block, 0, st, d_data, d_off, n, o.status, o.flags, o.spans, o.rewrite_begin);
    } else {
        lcNoteKernel("clog_docker_kernel");
        hipLaunchKernelGGL(lcclog::clog_docker_kernel, grid, block, 0, st, d_data, d_off, n, o.status, o.flags, o.spans, o.rewrite_begin, d_shadow);
    }
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

static bool formatKnown(int format) { return format == LC_CLOG_CONTAINERD || format == LC_CLOG_DOCKER; }
static bool outComplete(const lc_clog_out_t* o) { return o && o->status && o->flags && o->spans && o->rewrite_begin; }
// aligned for the stores the kernels make (spans: three 8-byte vectors per line)
static bool outAligned(const lc_clog_out_t& o) {
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    return !(misaligned(o.spans, 8) || misaligned(o.rewrite_begin, 4));
}

extern "C" int lc_container_log_parse_device(int format, const uint8_t* d_data, const int32_t* d_off, uint32_t n, const lc_clog_out_t* d_out,
                                             uint8_t* d_shadow, void* stream) {
    if (!formatKnown(format)) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !outComplete(d_out) || !outAligned(*d_out) || (format == LC_CLOG_DOCKER && !d_shadow)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the container log parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchParse(format, d_data, d_off, n, *d_out, d_shadow, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines
namespace {
struct ClogThread : PackedShadowBuffers<ClogThread> {
    ~ClogThread() {
        if (live()) release();
    }
    void release() { releaseBuffers(); }
};
thread_local ClogThread tlsClog;
}  // namespace

void lcClogThreadRelease() { tlsClog.release(); }

extern "C" int lc_container_log_parse_host(int format, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const lc_clog_out_t* out,
                                           uint8_t* shadow, uint64_t* shadow_bytes_moved) {
    if (shadow_bytes_moved) *shadow_bytes_moved = 0;
    if (!formatKnown(format)) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    const bool docker = format == LC_CLOG_DOCKER;
    if (!lines || !len || !outComplete(out) || (docker && !shadow)) return LC_ERR_ARG;
    ClogThread& T = tlsClog;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the container log parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    // a chunk: 32 MiB of payload, 2^18 lines, 64 MiB of results; down come spans, rewrite_begin, status, flags
    const PackedTripSpec spec{"lc_container_log_parse_host", "line", 1u << 18, 32u << 20, 24 + 4 + 1 + 1, 64u << 20,
                              "hipMemcpyAsync(container log results)"};
    enum { kSpans, kRewrite, kStatus, kFlags };
    return packedTrip(
        T, spec, lines, len, n, {24, 4, 1, 1},
        [&](const PackedChunk& c) {
            const size_t offAt = c.in.offAt;
            if (docker) LC_HIP_TRY(T.dShadow.ensure(offAt));
            const lc_clog_out_t d{c.dResult<uint8_t>(kStatus), c.dResult<uint8_t>(kFlags), c.dResult<int32_t>(kSpans), c.dResult<int32_t>(kRewrite)};
            return launchParse(format, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + offAt), c.cnt, d, static_cast<uint8_t*>(T.dShadow.p), T.stream);
        },
        [&](PackedChunk& c) {
            std::memcpy(out->spans + size_t(c.next) * 6, c.hResult(kSpans, 24), size_t(c.cnt) * 24);
            std::memcpy(out->rewrite_begin + c.next, c.hResult(kRewrite, 4), size_t(c.cnt) * 4);
            std::memcpy(out->status + c.next, c.hResult(kStatus, 1), c.cnt);
            std::memcpy(out->flags + c.next, c.hResult(kFlags, 1), c.cnt);
            // the unescaped bytes: only [rewrite_begin, content end) of the rewritten lines come down.  (A line flagged LC_CLOG_REPLAY is
            // finished by the host routine: nothing of it is moved.)
            std::vector<TripRange> spans;
            for (uint32_t i = 0; docker && i < c.cnt; ++i) {
                const uint32_t li = c.next + i;
                if (out->status[li] == LC_CLOG_FAIL_JSON || (out->flags[li] & (LC_CLOG_ESCAPED | LC_CLOG_REPLAY)) != LC_CLOG_ESCAPED) continue;
                const size_t at = size_t(c.hOff()[i]);
                const TripRange r{at + size_t(out->rewrite_begin[li]), at + size_t(out->spans[size_t(li) * 6 + 5])};
                if (r.e > r.b) spans.push_back(r);
            }
            return packedShadowDown(T, &c, spans, shadow, "hipMemcpyAsync(container log unescaped bytes)");
        },
        shadow_bytes_moved);
}
