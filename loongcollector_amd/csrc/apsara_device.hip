// apsara_device.hip -- the engine level of the Apsara parser (include/lc_apsara.h): the launch of apsara_parse_kernel
// (apsara_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/lc_apsara.h"
#include "apsara_kernel.hpp"
#include "packed_trip.hpp"

static int launchParse(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, const lc_apsara_out_t& o, hipStream_t st) {
    const dim3 grid((n + lcapsara::kBlock - 1) / lcapsara::kBlock), block(lcapsara::kBlock);
    lcNoteKernel("apsara_parse_kernel");
    hipLaunchKernelGGL(lcapsara::apsara_parse_kernel, grid, block, 0, st, d_data, d_off, n, W, o.status, o.secs, o.nanos, o.base, o.npairs, o.pairs);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

static bool outComplete(const lc_apsara_out_t* o, uint32_t W) {
    return o && o->status && o->secs && o->nanos && o->base && o->npairs && (!W || o->pairs);
}
// aligned for the stores the kernel makes (base: two 16-byte vectors per line)
static bool outAligned(const lc_apsara_out_t& o, uint32_t W) {
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    return !(misaligned(o.base, 16) || misaligned(o.secs, 8) || misaligned(o.nanos, 4) || misaligned(o.npairs, 4) || (W && misaligned(o.pairs, 4)));
}

extern "C" int lc_apsara_parse_device(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, const lc_apsara_out_t* d_out,
                                      void* stream) {
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !outComplete(d_out, W) || !outAligned(*d_out, W)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the Apsara parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchParse(d_data, d_off, n, W, *d_out, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines
namespace {
thread_local PackedThread<struct ApsaraTag> tlsApsara;
}  // namespace

void lcApsaraThreadRelease() { tlsApsara.release(); }

extern "C" int lc_apsara_parse_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, const lc_apsara_out_t* out) {
    if (n == 0) return LC_OK;
    if (!lines || !len || !outComplete(out, W)) return LC_ERR_ARG;
    auto& T = tlsApsara;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the Apsara parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t linePairBytes = size_t(W) * sizeof(ApsaraPair);
    // a chunk: 32 MiB of payload, 2^18 lines, 64 MiB of results; down come pairs, base, secs, nanos, npairs, status
    const PackedTripSpec spec{"lc_apsara_parse_host", "line", 1u << 18, 32u << 20, linePairBytes + 32 + 8 + 4 + 4 + 1, 64u << 20,
                              "hipMemcpyAsync(Apsara results)"};
    enum { kPairs, kBase, kSecs, kNanos, kNpairs, kStatus };
    return packedTrip(
        T, spec, lines, len, n, {linePairBytes, 32, 8, 4, 4, 1},
        [&](const PackedChunk& c) {
            // (with W short of a line's pairs the pair block is only partly written: the copy down moves it whole, the caller reads
            // min(npairs, W) entries of a line)
            const lc_apsara_out_t d{c.dResult<uint8_t>(kStatus), c.dResult<int64_t>(kSecs),    c.dResult<uint32_t>(kNanos),
                                    c.dResult<int32_t>(kBase),   c.dResult<uint32_t>(kNpairs), c.dResult<int32_t>(kPairs)};
            return launchParse(c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, W, d, T.stream);
        },
        [&](PackedChunk& c) {
            const uint32_t* np = reinterpret_cast<const uint32_t*>(c.hResult(kNpairs, 4));
            const uint8_t* hPairs = c.hResult(kPairs, linePairBytes);
            for (uint32_t i = 0; W && i < c.cnt; ++i) {  // only what the kernel wrote: the caller's array keeps what it held behind it
                const uint32_t k = np[i] < W ? np[i] : W;
                if (k) std::memcpy(out->pairs + (size_t(c.next) + i) * W * 3, hPairs + size_t(i) * linePairBytes, size_t(k) * sizeof(ApsaraPair));
            }
            std::memcpy(out->base + size_t(c.next) * 8, c.hResult(kBase, 32), size_t(c.cnt) * 32);
            std::memcpy(out->secs + c.next, c.hResult(kSecs, 8), size_t(c.cnt) * 8);
            std::memcpy(out->nanos + c.next, c.hResult(kNanos, 4), size_t(c.cnt) * 4);
            std::memcpy(out->npairs + c.next, np, size_t(c.cnt) * 4);
            std::memcpy(out->status + c.next, c.hResult(kStatus, 1), c.cnt);
            return LC_OK;
        });
}
