// anchor_device.hip -- the engine level of the anchor processor (include/anchor/lc_anchor.h): the launch of anchor_locate_kernel
// (anchor_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.  The handle and everything the Go plugin does
// around the search live in processor_anchor_gpu.cpp.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/anchor/lc_anchor.h"
#include "anchor_kernel.hpp"
#include "packed_trip.hpp"
#include "processor_anchor_gpu.hpp"

static int launchLocate(const AnchorConfig& cfg, const uint8_t* d_data, const int32_t* d_off, uint32_t n, int32_t* d_spans, hipStream_t st) {
    const dim3 grid((n + lcanchor::kBlock - 1) / lcanchor::kBlock), block(lcanchor::kBlock);
    const uint32_t S = anchorStride(cfg);
    lcNoteKernel("anchor_locate_kernel");
    hipLaunchKernelGGL(lcanchor::anchor_locate_kernel, grid, block, 0, st, cfg, d_data, d_off, n, S, d_spans);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// ProcessAnchor's searches (anchor.go:172-199) for n values at once
extern "C" int lc_anchor_locate_device(const lc_anchor_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, int32_t* d_spans, void* stream) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_spans) return LC_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_spans) & 15u) return LC_ERR_ARG;  // a row is whole 16-byte units
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the anchor processor has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    if (lcAnchorConfig(p).count == 0) return LC_OK;  // no anchors: rows of no entries
    return launchLocate(lcAnchorConfig(p), d_data, d_off, n, d_spans, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
thread_local PackedThread<struct AnchorTag> tlsAnchor;
}  // namespace

extern "C" void lc_anchor_thread_release(void) { tlsAnchor.release(); }

extern "C" int lc_anchor_locate_host(const lc_anchor_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, int32_t* spans) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !spans) return LC_ERR_ARG;
    auto& T = tlsAnchor;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the anchor processor has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const AnchorConfig& cfg = lcAnchorConfig(p);
    if (cfg.count == 0) return LC_OK;
    const size_t rowBytes = size_t(anchorStride(cfg)) * 8;
    // a chunk: 32 MiB of payload, 2^18 values, 64 MiB of rows; down come the rows
    const PackedTripSpec spec{"lc_anchor_locate_host", "value", 1u << 18, 32u << 20, rowBytes, 64u << 20, "hipMemcpyAsync(anchor rows)"};
    return packedTrip(
        T, spec, lines, len, n, {rowBytes},
        [&](const PackedChunk& c) {
            return launchLocate(cfg, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, c.dResult<int32_t>(0), T.stream);
        },
        [&](PackedChunk& c) {
            std::memcpy(reinterpret_cast<uint8_t*>(spans) + size_t(c.next) * rowBytes, c.hResult(0, rowBytes), size_t(c.cnt) * rowBytes);
            return LC_OK;
        });
}
