// sls_device.hip -- the engine level of the SLS encoder (include/sls/lc_sls.h): a plan's copy on a device, the launches of
// sls_kernel.hpp and the host entry's one trip through a runner thread's pinned staging.  The plan itself and the tags are
// sls_plan.cpp's, the processor level is processor_sls_gpu.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sls/lc_sls.h"
#include "runtime_internal.hpp"
#include "sls_kernel.hpp"
#include "sls_plan.hpp"
#include "trip_buffers.hpp"

using lcsls::SlsBatch;
using lcsls::SlsPlanView;

namespace {
constexpr uint32_t kWriteLanes = 8;  // lanes per event in sls_write_kernel (DESIGN.md section 5.17 has the figures of 4 to 64)

uint32_t scanTiles(uint32_t n) { return uint32_t((uint64_t(n) + 1 + lcsls::kScanTile - 1) / lcsls::kScanTile); }

void releasePlanCopies(lc_sls_plan* plan) {
    if (!lcRuntimeUsable()) return;
    for (const lc_sls_plan::OnDevice& d : plan->onDevice) (void)hipFree(d.block);  // (a pointer names its device)
    plan->onDevice.clear();
}

// the plan's tables on `dev` (the current device): uploaded at first use
int planOnDevice(lc_sls_plan* plan, int dev, SlsPlanView* view) {
    const size_t itemBytes = tripRoundUp(plan->items.size() * sizeof(lcsls::SlsItem), 16);
    std::lock_guard<std::mutex> g(plan->mu);
    void* block = nullptr;
    for (const lc_sls_plan::OnDevice& d : plan->onDevice)
        if (d.dev == dev) block = d.block;
    if (!block) {
        LC_HIP_TRY(hipMalloc(&block, itemBytes + plan->blob.size()));
        hipError_t e = hipMemcpy(block, plan->items.data(), plan->items.size() * sizeof(lcsls::SlsItem), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(static_cast<uint8_t*>(block) + itemBytes, plan->blob.data(), plan->blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(block);
            return lcHipFail(e, "hipMemcpy(the SLS plan's tables)");
        }
        plan->onDevice.push_back({dev, block});
        plan->releaseDevice = releasePlanCopies;
    }
    view->items = static_cast<const lcsls::SlsItem*>(block);
    view->blob = static_cast<const uint8_t*>(block) + itemBytes;
    view->nMatched = plan->nMatched;
    view->nUnmatched = plan->nUnmatched;
    return LC_OK;
}

// totalOut: where the kernel also leaves rec_off[n] (a pinned word of the host entry's trip), or null
int launchWrite(const SlsPlanView& P, const SlsBatch& b, const uint64_t* dRecOff, uint8_t* dOut, uint64_t outCap, uint64_t* totalOut, hipStream_t st) {
    const uint64_t lanes = uint64_t(b.n) * kWriteLanes;
    lcNoteKernel("sls_write_kernel");
    hipLaunchKernelGGL(lcsls::sls_write_kernel<kWriteLanes>, dim3(uint32_t((lanes + lcsls::kBlock - 1) / lcsls::kBlock)), dim3(lcsls::kBlock), 0, st, P, b,
                       dRecOff, dOut, outCap, totalOut);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// size, scan, write: everything lc_sls_encode_device queues
int encodeOnStream(const SlsPlanView& P, const SlsBatch& b, uint8_t* dOut, uint64_t outCap, uint64_t* dRecOff, void* dScratch, uint64_t* totalOut,
                   hipStream_t st) {
    const uint32_t m = b.n + 1, tiles = scanTiles(b.n);
    uint64_t* tileSums = static_cast<uint64_t*>(dScratch);
    lcNoteKernel("sls_size_kernel");
    hipLaunchKernelGGL(lcsls::sls_size_kernel, dim3((m + lcsls::kBlock - 1) / lcsls::kBlock), dim3(lcsls::kBlock), 0, st, P, b, dRecOff);
    LC_HIP_TRY(hipGetLastError());
    lcNoteKernel("sls_scan_kernel");
    if (tiles == 1) {  // (a group of an agent: one launch instead of three)
        hipLaunchKernelGGL(lcsls::sls_scan_apply_kernel, dim3(1), dim3(lcsls::kBlock), 0, st, dRecOff, m, static_cast<const uint64_t*>(nullptr));
    } else {
        hipLaunchKernelGGL(lcsls::sls_scan_sums_kernel, dim3(tiles), dim3(lcsls::kBlock), 0, st, dRecOff, m, tileSums);
        hipLaunchKernelGGL(lcsls::sls_scan_tiles_kernel, dim3(1), dim3(lcsls::kScanTilesPerPass), 0, st, tileSums, tiles);
        hipLaunchKernelGGL(lcsls::sls_scan_apply_kernel, dim3(tiles), dim3(lcsls::kBlock), 0, st, dRecOff, m, static_cast<const uint64_t*>(tileSums));
    }
    LC_HIP_TRY(hipGetLastError());
    return launchWrite(P, b, dRecOff, dOut, outCap, totalOut, st);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" size_t lc_sls_scratch_bytes(uint32_t n) { return tripRoundUp(size_t(scanTiles(n)) * 8, 256); }

extern "C" int lc_sls_encode_device(lc_sls_plan_t* plan, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t sep_bytes,
                                    uint32_t n, uint32_t ngroups, const int32_t* d_caps, const uint8_t* d_status, const uint32_t* d_time,
                                    const int32_t* d_time_ns, int enable_ns, uint8_t* d_out, uint64_t out_cap, uint64_t* d_rec_off, void* d_scratch,
                                    size_t scratch_bytes, void* stream) {
    if (!plan || !d_rec_off || !aligned(d_rec_off, 8)) return LC_ERR_ARG;
    if (n >= (1u << 31) || plan->maxSource > ngroups) return LC_ERR_ARG;
    if ((out_cap && !d_out) || !aligned(d_out, 16)) return LC_ERR_ARG;
    if (n && (!d_data || !d_off || !d_status || !d_time || (ngroups && !d_caps))) return LC_ERR_ARG;
    if (!aligned(d_off, 4) || !aligned(d_len, 4) || !aligned(d_caps, 4) || !aligned(d_time, 4) || !aligned(d_time_ns, 4)) return LC_ERR_ARG;
    if (!d_scratch || !aligned(d_scratch, 8) || scratch_bytes < lc_sls_scratch_bytes(n)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the SLS encoder has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(n ? static_cast<const void*>(d_data) : d_rec_off, &dev);  // (never switches devices)
    if (rcDev != LC_OK) return rcDev;
    if (n == 0) {
        LC_HIP_TRY(hipMemsetAsync(d_rec_off, 0, 8, static_cast<hipStream_t>(stream)));
        return LC_OK;
    }
    SlsPlanView P{};
    const int rcPlan = planOnDevice(plan, dev, &P);
    if (rcPlan != LC_OK) return rcPlan;
    const SlsBatch b{d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_time_ns, enable_ns ? 1u : 0u};
    return encodeOnStream(P, b, d_out, out_cap, d_rec_off, d_scratch, nullptr, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines: one trip
namespace {
struct SlsThread : TripThread<SlsThread> {
    TripBuf hIn, hOut, dIn, dWork;
    SlsThread() : TripThread<SlsThread>(true) { hIn.pinned = hOut.pinned = true; }
    ~SlsThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dWork}); }
};
thread_local SlsThread tlsSls;
}  // namespace

extern "C" void lc_sls_thread_release(void) { tlsSls.release(); }

extern "C" int lc_sls_match_encode_host(lc_sls_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
                                        const uint32_t* time, const int32_t* time_ns, int enable_ns, const uint8_t** out, size_t* out_len,
                                        uint64_t* rec_off, uint8_t* status) {
    if (!plan || !re || !out || !out_len) return LC_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    if (n == 0) {
        if (rec_off) rec_off[0] = 0;
        return LC_OK;
    }
    if (!lines || !len || !time || !status || n >= (1u << 31)) return LC_ERR_ARG;
    const uint32_t G = uint32_t(lc_regex_mark_count(re));
    if (plan->maxSource > G) return LC_ERR_ARG;
    SlsThread& T = tlsSls;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the SLS encoder has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    uint64_t payload = 0;
    for (uint32_t i = 0; i < n; ++i) payload += len[i];
    if (payload >= (1ull << 31)) {
        lcSetLastError("lc_sls_match_encode_host: 2 GiB of lines or more in one call");
        return LC_ERR_ARG;
    }
    // up: the lines back to back, their n + 1 offsets, the times, the nanosecond parts -- one block, pulled by a kernel
    const bool ns = enable_ns && time_ns;
    const size_t offAt = tripOffAt(payload), timeAt = offAt + tripRoundUp((size_t(n) + 1) * 4, 16), nsAt = timeAt + tripRoundUp(size_t(n) * 4, 16);
    const size_t inBytes = tripRoundUp(nsAt + (ns ? size_t(n) * 4 : 0), 16);
    // on the device: rows, record offsets, the scan's scratch
    const size_t recAt = tripRoundUp(size_t(n) * 2 * G * 4, 16);
    const size_t scratchAt = recAt + tripRoundUp((size_t(n) + 1) * 8, 16), scratchBytes = lc_sls_scratch_bytes(n);
    // No copy engine anywhere in the trip (its queue is shared by all runner threads): the kernels store what
    // the host needs -- the total, the status bytes, the records -- into ONE pinned block through its mapping.
    const size_t hStatusAt = 16, hPayloadAt = hStatusAt + tripRoundUp(n, 16);
    // what the records take when no line's rows overlap: the room the first write gets
    const uint64_t fixed = std::max(plan->boundFixed[0], plan->boundFixed[1]), perLine = std::max(plan->boundLines[0], plan->boundLines[1]);
    const uint64_t guess = tripRoundUp(uint64_t(n) * fixed + perLine * payload, 16);
    LC_HIP_TRY(T.hIn.ensure(inBytes));
    LC_HIP_TRY(T.dIn.ensure(inBytes));
    LC_HIP_TRY(T.dWork.ensure(scratchAt + scratchBytes));
    LC_HIP_TRY(T.hOut.ensure(hPayloadAt + guess));
    uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
    uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
    uint8_t* dWork = static_cast<uint8_t*>(T.dWork.p);
    uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
    tripPackLines(hIn, offAt, lines, len, 0, n);
    reinterpret_cast<uint32_t*>(hIn + offAt)[n] = uint32_t(payload);
    std::memcpy(hIn + timeAt, time, size_t(n) * 4);
    if (ns) std::memcpy(hIn + nsAt, time_ns, size_t(n) * 4);
    SlsPlanView P{};
    int rc = planOnDevice(plan, dev, &P);
    if (rc != LC_OK) return rc;
    const SlsBatch b{dIn, reinterpret_cast<const uint32_t*>(dIn + offAt), nullptr, 0, n, G, reinterpret_cast<const int32_t*>(dWork), hOut + hStatusAt,
                     reinterpret_cast<const uint32_t*>(dIn + timeAt), ns ? reinterpret_cast<const int32_t*>(dIn + nsAt) : nullptr, ns ? 1u : 0u};
    uint64_t* dRecOff = reinterpret_cast<uint64_t*>(dWork + recAt);
    uint64_t* hTotal = reinterpret_cast<uint64_t*>(hOut);
    const uint64_t cap = T.hOut.cap - hPayloadAt;
    rc = lc_upload_pinned(hIn, dIn, inBytes, T.stream);
    if (rc == LC_OK) rc = lc_regex_match_device(re, dIn, b.off, nullptr, 0, n, G, reinterpret_cast<int32_t*>(dWork), hOut + hStatusAt, T.stream);
    if (rc == LC_OK) rc = encodeOnStream(P, b, hOut + hPayloadAt, cap, dRecOff, dWork + scratchAt, hTotal, T.stream);
    if (rc == LC_OK && rec_off) {  // (only a caller that asks for the offsets pays a copy)
        const hipError_t e = hipMemcpyAsync(rec_off, dRecOff, (size_t(n) + 1) * 8, hipMemcpyDeviceToHost, T.stream);
        if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(SLS record offsets)");
    }
    rc = T.end(rc);
    if (rc != LC_OK) return rc;
    const uint64_t total = *hTotal;
    std::memcpy(status, hOut + hStatusAt, n);
    if (total > cap) {
        // rows that overlap (nested groups, the line beside its groups): the write once more, into a block with room for all of it
        // (the pinned block moves: the status bytes are with the caller already)
        LC_HIP_TRY(T.hOut.ensure(hPayloadAt + total));
        hOut = static_cast<uint8_t*>(T.hOut.p);
        std::memcpy(hOut + hStatusAt, status, n);
        SlsBatch again = b;
        again.status = hOut + hStatusAt;
        rc = T.end(launchWrite(P, again, dRecOff, hOut + hPayloadAt, T.hOut.cap - hPayloadAt, reinterpret_cast<uint64_t*>(hOut), T.stream));
        if (rc != LC_OK) return rc;
    }
    *out = hOut + hPayloadAt;
    *out_len = size_t(total);
    return LC_OK;
}
