// apsara_device.hip -- the engine level of the Apsara parser (include/lc_apsara.h): the launch of apsara_parse_kernel
// (apsara_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/lc_apsara.h"
#include "apsara_kernel.hpp"
#include "runtime_internal.hpp"
#include "trip_buffers.hpp"

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
// per runner thread: a stream, one pinned and one device block each way, the pinned completion word; grow-only
struct ApsaraThread : TripThread<ApsaraThread> {
    TripBuf hIn, hOut, dIn, dOut;
    ApsaraThread() : TripThread(true) { hIn.pinned = hOut.pinned = true; }
    ~ApsaraThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dOut}); }
};
thread_local ApsaraThread tlsApsara;

constexpr size_t kChunkBytes = 32u << 20;    // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;   // and at most this many lines
constexpr size_t kChunkResultBytes = 64u << 20;
constexpr size_t kFixedResultBytes = 32 + 8 + 4 + 4 + 1;  // base, secs, nanos, npairs, status
}  // namespace

void lcApsaraThreadRelease() { tlsApsara.release(); }

extern "C" int lc_apsara_parse_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, const lc_apsara_out_t* out) {
    if (n == 0) return LC_OK;
    if (!lines || !len || !outComplete(out, W)) return LC_ERR_ARG;
    ApsaraThread& T = tlsApsara;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the Apsara parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t linePairBytes = size_t(W) * sizeof(ApsaraPair);
    uint32_t next = 0;
    while (next < n) {
        // a chunk: the lines back to back, then (64-byte aligned) their n + 1 offsets -- ONE copy up; every result array in one device
        // block -- ONE copy down
        uint32_t cnt = 0;
        size_t bytes = 0;
        if (!tripCarve(len, next, n, kChunkLines, kChunkBytes, linePairBytes + kFixedResultBytes, kChunkResultBytes, &cnt, &bytes)) {
            lcSetLastError("lc_apsara_parse_host: a line of 2 GiB or more");
            return LC_ERR_ARG;
        }
        const size_t offAt = tripOffAt(bytes);
        const size_t inBytes = offAt + (size_t(cnt) + 1) * 4;
        const size_t baseAt = tripRoundUp(size_t(cnt) * linePairBytes, 64);
        const size_t secsAt = baseAt + tripRoundUp(size_t(cnt) * 32, 64);
        const size_t nanosAt = secsAt + tripRoundUp(size_t(cnt) * 8, 64);
        const size_t npairsAt = nanosAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t statusAt = npairsAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t outBytes = statusAt + tripRoundUp(cnt, 64);
        LC_HIP_TRY(T.hIn.ensure(inBytes));
        LC_HIP_TRY(T.dIn.ensure(inBytes));
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
        reinterpret_cast<int32_t*>(hIn + offAt)[cnt] = int32_t(tripPackLines(hIn, offAt, lines, len, next, cnt));
        uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
        uint8_t* dOut = static_cast<uint8_t*>(T.dOut.p);
        LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
        const lc_apsara_out_t d{dOut + statusAt, reinterpret_cast<int64_t*>(dOut + secsAt), reinterpret_cast<uint32_t*>(dOut + nanosAt),
                                reinterpret_cast<int32_t*>(dOut + baseAt), reinterpret_cast<uint32_t*>(dOut + npairsAt),
                                reinterpret_cast<int32_t*>(dOut)};
        int rc = launchParse(dIn, reinterpret_cast<const int32_t*>(dIn + offAt), cnt, W, d, T.stream);
        // (with W short of a line's pairs the pair block is only partly written: the copy down moves it whole, the caller reads
        // min(npairs, W) entries of a line)
        if (rc == LC_OK) {
            const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(Apsara results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint8_t* hOut = static_cast<const uint8_t*>(T.hOut.p);
        const uint32_t* np = reinterpret_cast<const uint32_t*>(hOut + npairsAt);
        for (uint32_t i = 0; W && i < cnt; ++i) {  // only what the kernel wrote: the caller's array keeps what it held behind it
            const uint32_t k = np[i] < W ? np[i] : W;
            if (k) std::memcpy(out->pairs + (size_t(next) + i) * W * 3, hOut + size_t(i) * linePairBytes, size_t(k) * sizeof(ApsaraPair));
        }
        std::memcpy(out->base + size_t(next) * 8, hOut + baseAt, size_t(cnt) * 32);
        std::memcpy(out->secs + next, hOut + secsAt, size_t(cnt) * 8);
        std::memcpy(out->nanos + next, hOut + nanosAt, size_t(cnt) * 4);
        std::memcpy(out->npairs + next, np, size_t(cnt) * 4);
        std::memcpy(out->status + next, hOut + statusAt, cnt);
        next += cnt;
    }
    return LC_OK;
}
