// jsonl_device.hip -- the engine level of the JSON-lines encoder (include/jsonl/lc_jsonl.h): a plan's copy on a device, the launches
// of jsonl_kernel.hpp and scan64_kernel.hpp, and the host entry's one trip through a runner thread's pinned staging.  The plan itself
// and the head are jsonl_plan.cpp's, the processor level is processor_jsonl_gpu.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/jsonl/lc_jsonl.h"
#include "jsonl_kernel.hpp"
#include "jsonl_plan.hpp"
#include "runtime_internal.hpp"
#include "scan64_kernel.hpp"
#include "trip_buffers.hpp"

using lcjsonl::JsonlBatch;
using lcjsonl::JsonlPlanView;

namespace {
// lanes per event, one instantiation per kernel: the size pass is fastest with four, the write pass with eight (DESIGN.md section
// 5.20 has the figures of 4 to 32).  (-DLC_JSONL_LANES=4 .. 64 builds both kernels at one width: the variants tools/jsonl_bench.py
// --lib measures)
#ifdef LC_JSONL_LANES
constexpr uint32_t kSizeLanes = LC_JSONL_LANES, kWriteLanes = LC_JSONL_LANES;
#else
constexpr uint32_t kSizeLanes = 4, kWriteLanes = 8;
#endif
constexpr uint32_t kLanes = kSizeLanes > kWriteLanes ? kSizeLanes : kWriteLanes;
static_assert(kSizeLanes >= 2 && kLanes <= 64 && (kSizeLanes & (kSizeLanes - 1)) == 0 && (kWriteLanes & (kWriteLanes - 1)) == 0,
              "lanes per event: a power of two, 2 .. 64");

size_t tileSumRoom(uint32_t n) { return tripRoundUp(lcscan::tileSumBytes(uint64_t(n) + 1), 256); }

void releasePlanCopies(lc_jsonl_plan* plan) {
    if (!lcRuntimeUsable()) return;
    for (const lc_jsonl_plan::OnDevice& d : plan->onDevice) (void)hipFree(d.block);  // (a pointer names its device)
    plan->onDevice.clear();
}

// the plan's tables on `dev` (the current device): uploaded at first use
int planOnDevice(lc_jsonl_plan* plan, int dev, JsonlPlanView* view) {
    const size_t itemBytes = tripRoundUp(plan->items.size() * sizeof(lcjsonl::JsonlItem), 16);
    std::lock_guard<std::mutex> g(plan->mu);
    void* block = nullptr;
    for (const lc_jsonl_plan::OnDevice& d : plan->onDevice)
        if (d.dev == dev) block = d.block;
    if (!block) {
        LC_HIP_TRY(hipMalloc(&block, itemBytes + plan->blob.size()));
        hipError_t e = hipMemcpy(block, plan->items.data(), plan->items.size() * sizeof(lcjsonl::JsonlItem), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(static_cast<uint8_t*>(block) + itemBytes, plan->blob.data(), plan->blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(block);
            return lcHipFail(e, "hipMemcpy(the JSON-lines plan's tables)");
        }
        plan->onDevice.push_back({dev, block});
        plan->releaseDevice = releasePlanCopies;
    }
    view->items = static_cast<const lcjsonl::JsonlItem*>(block);
    view->blob = static_cast<const uint8_t*>(block) + itemBytes;
    view->nMatched = plan->nMatched;
    view->nUnmatched = plan->nUnmatched;
    return LC_OK;
}

uint32_t blocksFor(uint64_t events, uint32_t lanes) { return uint32_t((events * lanes + lcjsonl::kBlock - 1) / lcjsonl::kBlock); }

// totalOut: where the kernel also leaves rec_off[n] (a pinned word of the host entry's trip), or null
int launchWrite(const JsonlPlanView& P, const JsonlBatch& b, const uint64_t* dRecOff, const uint32_t* itemLens, uint8_t* dOut, uint64_t outCap,
                uint64_t* totalOut, hipStream_t st) {
    lcNoteKernel("jsonl_write_kernel");
    hipLaunchKernelGGL(lcjsonl::jsonl_write_kernel<kWriteLanes>, dim3(blocksFor(b.n, kWriteLanes)), dim3(lcjsonl::kBlock), 0, st, P, b, dRecOff, itemLens, dOut, outCap,
                       totalOut);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// where the size pass leaves (raw length, escaped length) per item for the write pass.  (-DLC_JSONL_REDERIVE builds the variant whose
// write pass classifies the values again instead: measured slower)
uint32_t* itemLensIn(void* dScratch, uint32_t n) {
#ifdef LC_JSONL_REDERIVE
    return nullptr;
#else
    return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(dScratch) + tileSumRoom(n));
#endif
}

// size, scan, write: everything lc_jsonl_encode_device queues
int encodeOnStream(const JsonlPlanView& P, const JsonlBatch& b, uint8_t* dOut, uint64_t outCap, uint64_t* dRecOff, void* dScratch, uint64_t* totalOut,
                   hipStream_t st) {
    uint32_t* itemLens = itemLensIn(dScratch, b.n);
    lcNoteKernel("jsonl_size_kernel");
    hipLaunchKernelGGL(lcjsonl::jsonl_size_kernel<kSizeLanes>, dim3(blocksFor(uint64_t(b.n) + 1, kSizeLanes)), dim3(lcjsonl::kBlock), 0, st, P, b, dRecOff, itemLens);
    LC_HIP_TRY(hipGetLastError());
    lcNoteKernel("scan64_kernel");
    LC_HIP_TRY(lcscan::exclusiveScan(dRecOff, b.n + 1, static_cast<uint64_t*>(dScratch), st));
    return launchWrite(P, b, dRecOff, itemLens, dOut, outCap, totalOut, st);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool headLenServed(uint32_t headLen) { return headLen >= lcjsonl::kMinHeadBytes && headLen <= LC_JSONL_MAX_HEAD_BYTES; }
}  // namespace

extern "C" size_t lc_jsonl_scratch_bytes(const lc_jsonl_plan_t* plan, uint32_t n) {
    if (!plan) return 0;
    return tileSumRoom(n) + tripRoundUp(size_t(n) * plan->itemStride() * 8, 256);
}

extern "C" int lc_jsonl_encode_device(lc_jsonl_plan_t* plan, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t sep_bytes,
                                      uint32_t n, uint32_t ngroups, const int32_t* d_caps, const uint8_t* d_status, const uint32_t* d_time,
                                      const uint8_t* d_head, uint32_t head_len, uint8_t* d_out, uint64_t out_cap, uint64_t* d_rec_off,
                                      void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!plan || !d_rec_off || !aligned(d_rec_off, 8)) return LC_ERR_ARG;
    if (n >= (1u << 31) || plan->maxSource > ngroups) return LC_ERR_ARG;
    if ((out_cap && !d_out) || !aligned(d_out, 16)) return LC_ERR_ARG;
    if (n && (!d_data || !d_off || !d_status || !d_time || (ngroups && !d_caps))) return LC_ERR_ARG;
    if (!d_head || !aligned(d_head, 4) || !headLenServed(head_len)) return LC_ERR_ARG;
    if (!aligned(d_off, 4) || !aligned(d_len, 4) || !aligned(d_caps, 4) || !aligned(d_time, 4)) return LC_ERR_ARG;
    if (!d_scratch || !aligned(d_scratch, 8) || scratch_bytes < lc_jsonl_scratch_bytes(plan, n)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the JSON-lines encoder has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(n ? static_cast<const void*>(d_data) : d_rec_off, &dev);  // (never switches devices)
    if (rcDev != LC_OK) return rcDev;
    if (n == 0) {
        LC_HIP_TRY(hipMemsetAsync(d_rec_off, 0, 8, static_cast<hipStream_t>(stream)));
        return LC_OK;
    }
    JsonlPlanView P{};
    const int rcPlan = planOnDevice(plan, dev, &P);
    if (rcPlan != LC_OK) return rcPlan;
    const JsonlBatch b{d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_head, head_len, plan->itemStride()};
    return encodeOnStream(P, b, d_out, out_cap, d_rec_off, d_scratch, nullptr, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines: one trip
namespace {
struct JsonlThread : TripThread<JsonlThread> {
    TripBuf hIn, hOut, dIn, dWork;
    JsonlThread() : TripThread<JsonlThread>(true) { hIn.pinned = hOut.pinned = true; }
    ~JsonlThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dWork}); }
};
thread_local JsonlThread tlsJsonl;
}  // namespace

extern "C" void lc_jsonl_thread_release(void) { tlsJsonl.release(); }

extern "C" int lc_jsonl_match_encode_host(lc_jsonl_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
                                          const uint32_t* time, const uint8_t* head, uint32_t head_len, const uint8_t** out, size_t* out_len,
                                          uint64_t* rec_off, uint8_t* status) {
    if (!plan || !re || !out || !out_len) return LC_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    if (n == 0) {
        if (rec_off) rec_off[0] = 0;
        return LC_OK;
    }
    if (!lines || !len || !time || !status || !head || !headLenServed(head_len) || n >= (1u << 31)) return LC_ERR_ARG;
    const uint32_t G = uint32_t(lc_regex_mark_count(re));
    if (plan->maxSource > G) return LC_ERR_ARG;
    JsonlThread& T = tlsJsonl;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the JSON-lines encoder has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    uint64_t payload = 0;
    for (uint32_t i = 0; i < n; ++i) payload += len[i];
    if (payload >= (1ull << 31)) {
        lcSetLastError("lc_jsonl_match_encode_host: 2 GiB of lines or more in one call");
        return LC_ERR_ARG;
    }
    // up: the lines back to back, their n + 1 offsets, the times, the head -- one block, pulled by a kernel
    const size_t offAt = tripOffAt(payload), timeAt = offAt + tripRoundUp((size_t(n) + 1) * 4, 16), headAt = timeAt + tripRoundUp(size_t(n) * 4, 16);
    const size_t inBytes = tripRoundUp(headAt + head_len, 16);
    // on the device: rows, record offsets, the scan's and the size pass's scratch
    const size_t recAt = tripRoundUp(size_t(n) * 2 * G * 4, 16);
    const size_t scratchAt = tripRoundUp(recAt + tripRoundUp((size_t(n) + 1) * 8, 16), 256), scratchBytes = lc_jsonl_scratch_bytes(plan, n);
    // No copy engine anywhere in the trip (its queue is shared by all runner threads): the kernels store what
    // the host needs -- the total, the status bytes, the records -- into ONE pinned block through its mapping.
    const size_t hStatusAt = 16, hPayloadAt = hStatusAt + tripRoundUp(n, 16);
    // what the records take when no line's rows overlap and no value holds a reactive byte: the room the first write gets
    const uint64_t fixed = head_len + std::max(plan->boundFixed[0], plan->boundFixed[1]), perLine = std::max(plan->boundLines[0], plan->boundLines[1]);
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
    std::memcpy(hIn + headAt, head, head_len);
    JsonlPlanView P{};
    int rc = planOnDevice(plan, dev, &P);
    if (rc != LC_OK) return rc;
    const JsonlBatch b{dIn, reinterpret_cast<const uint32_t*>(dIn + offAt), nullptr, 0, n, G, reinterpret_cast<const int32_t*>(dWork), hOut + hStatusAt,
                       reinterpret_cast<const uint32_t*>(dIn + timeAt), dIn + headAt, head_len, plan->itemStride()};
    uint64_t* dRecOff = reinterpret_cast<uint64_t*>(dWork + recAt);
    uint64_t* hTotal = reinterpret_cast<uint64_t*>(hOut);
    const uint64_t cap = T.hOut.cap - hPayloadAt;
    rc = lc_upload_pinned(hIn, dIn, inBytes, T.stream);
    if (rc == LC_OK) rc = lc_regex_match_device(re, dIn, b.off, nullptr, 0, n, G, reinterpret_cast<int32_t*>(dWork), hOut + hStatusAt, T.stream);
    if (rc == LC_OK) rc = encodeOnStream(P, b, hOut + hPayloadAt, cap, dRecOff, dWork + scratchAt, hTotal, T.stream);
    if (rc == LC_OK && rec_off) {  // (only a caller that asks for the offsets pays a copy)
        const hipError_t e = hipMemcpyAsync(rec_off, dRecOff, (size_t(n) + 1) * 8, hipMemcpyDeviceToHost, T.stream);
        if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(JSON-lines record offsets)");
    }
    rc = T.end(rc);
    if (rc != LC_OK) return rc;
    const uint64_t total = *hTotal;
    std::memcpy(status, hOut + hStatusAt, n);
    if (total > cap) {
        // reactive bytes, or rows that overlap: the write once more, into a block with room for all of it (the pinned block moves: the
        // status bytes are with the caller already; the size pass's item lengths still lie in the device's scratch)
        LC_HIP_TRY(T.hOut.ensure(hPayloadAt + total));
        hOut = static_cast<uint8_t*>(T.hOut.p);
        std::memcpy(hOut + hStatusAt, status, n);
        JsonlBatch again = b;
        again.status = hOut + hStatusAt;
        rc = T.end(launchWrite(P, again, dRecOff, itemLensIn(dWork + scratchAt, n), hOut + hPayloadAt, T.hOut.cap - hPayloadAt,
                               reinterpret_cast<uint64_t*>(hOut), T.stream));
        if (rc != LC_OK) return rc;
    }
    *out = hOut + hPayloadAt;
    *out_len = size_t(total);
    return LC_OK;
}
