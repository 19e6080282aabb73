// clog_device.hip -- the engine level of the container stdout parser (include/lc_container_log.h): the launches of
// clog_containerd_kernel / clog_docker_kernel (clog_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/lc_container_log.h"
#include "clog_kernel.hpp"
#include "runtime_internal.hpp"
#include "trip_buffers.hpp"

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
// per runner thread: a stream, pinned and device blocks each way, the pinned completion word; grow-only
struct ClogThread : TripThread<ClogThread> {
    TripBuf hIn, hOut, hShadow, dIn, dOut, dShadow;
    ClogThread() : TripThread(true) { hIn.pinned = hOut.pinned = hShadow.pinned = true; }
    ~ClogThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &hShadow, &dIn, &dOut, &dShadow}); }
};
thread_local ClogThread tlsClog;

constexpr size_t kChunkBytes = 32u << 20;   // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;  // and at most this many lines
constexpr size_t kChunkResultBytes = 64u << 20;
constexpr size_t kLineResultBytes = 24 + 4 + 1 + 1;  // spans, rewrite_begin, status, flags
constexpr uint32_t kShadowGap = 4096;                // two rewritten values closer than this come down in one copy
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
    uint32_t next = 0;
    size_t shadowAt = 0;  // where line `next`'s part of the caller's shadow begins
    uint64_t moved = 0;
    while (next < n) {
        // a chunk: the lines back to back, then (64-byte aligned) their n + 1 offsets -- ONE copy up; every result array in one device
        // block -- ONE copy down
        uint32_t cnt = 0;
        size_t bytes = 0;
        if (!tripCarve(len, next, n, kChunkLines, kChunkBytes, kLineResultBytes, kChunkResultBytes, &cnt, &bytes)) {
            lcSetLastError("lc_container_log_parse_host: a line of 2 GiB or more");
            return LC_ERR_ARG;
        }
        const size_t offAt = tripOffAt(bytes);
        const size_t inBytes = offAt + (size_t(cnt) + 1) * 4;
        const size_t rewriteAt = tripRoundUp(size_t(cnt) * 24, 64);
        const size_t statusAt = rewriteAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t flagsAt = statusAt + tripRoundUp(cnt, 64);
        const size_t outBytes = flagsAt + tripRoundUp(cnt, 64);
        LC_HIP_TRY(T.hIn.ensure(inBytes));
        LC_HIP_TRY(T.dIn.ensure(inBytes));
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        if (docker) LC_HIP_TRY(T.dShadow.ensure(offAt));
        uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
        int32_t* hOff = reinterpret_cast<int32_t*>(hIn + offAt);
        hOff[cnt] = int32_t(tripPackLines(hIn, offAt, lines, len, next, cnt));
        uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
        uint8_t* dOut = static_cast<uint8_t*>(T.dOut.p);
        uint8_t* dShadow = static_cast<uint8_t*>(T.dShadow.p);
        LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
        const lc_clog_out_t d{dOut + statusAt, dOut + flagsAt, reinterpret_cast<int32_t*>(dOut), reinterpret_cast<int32_t*>(dOut + rewriteAt)};
        int rc = launchParse(format, dIn, reinterpret_cast<const int32_t*>(dIn + offAt), cnt, d, dShadow, T.stream);
        if (rc == LC_OK) {
            const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(container log results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint8_t* hOut = static_cast<const uint8_t*>(T.hOut.p);
        std::memcpy(out->spans + size_t(next) * 6, hOut, size_t(cnt) * 24);
        std::memcpy(out->rewrite_begin + next, hOut + rewriteAt, size_t(cnt) * 4);
        std::memcpy(out->status + next, hOut + statusAt, cnt);
        std::memcpy(out->flags + next, hOut + flagsAt, cnt);
        if (docker) {
            // the unescaped bytes: only [rewrite_begin, content end) of the rewritten lines come down, neighbours within kShadowGap in
            // one copy.  (A line flagged LC_CLOG_REPLAY is finished by the host routine: nothing of it is moved.)
            struct Range {
                size_t b, e;
            };
            std::vector<Range> spans, copies;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint32_t li = next + i;
                if (out->status[li] == LC_CLOG_FAIL_JSON || (out->flags[li] & (LC_CLOG_ESCAPED | LC_CLOG_REPLAY)) != LC_CLOG_ESCAPED) continue;
                const Range r{size_t(hOff[i]) + size_t(out->rewrite_begin[li]), size_t(hOff[i]) + size_t(out->spans[size_t(li) * 6 + 5])};
                if (r.e <= r.b) continue;
                spans.push_back(r);
                if (!copies.empty() && r.b <= copies.back().e + kShadowGap) copies.back().e = r.e;
                else copies.push_back(r);
            }
            if (!copies.empty()) {
                LC_HIP_TRY(T.hShadow.ensure(offAt));
                uint8_t* hShadow = static_cast<uint8_t*>(T.hShadow.p);
                rc = LC_OK;
                for (const Range& c : copies) {
                    const hipError_t e = hipMemcpyAsync(hShadow + c.b, dShadow + c.b, c.e - c.b, hipMemcpyDeviceToHost, T.stream);
                    if (e != hipSuccess) {
                        rc = lcHipFail(e, "hipMemcpyAsync(container log unescaped bytes)");
                        break;
                    }
                    moved += c.e - c.b;
                }
                rc = T.end(rc);
                if (rc != LC_OK) return rc;
                for (const Range& r : spans) std::memcpy(shadow + shadowAt + r.b, hShadow + r.b, r.e - r.b);
            }
        }
        shadowAt += bytes;
        next += cnt;
    }
    if (shadow_bytes_moved) *shadow_bytes_moved = moved;
    return LC_OK;
}
