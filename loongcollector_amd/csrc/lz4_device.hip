// lz4_device.hip -- the LZ4 block writer's C ABI (include/lz4/lc_lz4.h): the launches of lz4_kernel.hpp, and the two host entries' one
// trip through a runner thread's pinned staging.  The regex match and the SLS records of the second entry are liblc_regex_gpu.so's and
// liblc_sls.so's own device entries, queued on the same stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/lz4/lc_lz4.h"
#include "lz4_kernel.hpp"
#include "runtime_internal.hpp"
#include "sls_plan.hpp"
#include "trip_buffers.hpp"

using lclz4::Lz4Job;

struct lc_lz4 {
    uint32_t chunk;
};

namespace {
#ifndef LC_LZ4_EMIT_LANES
#define LC_LZ4_EMIT_LANES 4  // (a build-time knob for the measurement of DESIGN.md section 5.19: 4, 8, 16 and 64 lanes)
#endif
constexpr uint32_t kDefaultChunk = 4096;             // DESIGN.md section 5.19 has the figures of 4, 16 and 64 KiB
constexpr uint32_t kEmitLanes = LC_LZ4_EMIT_LANES;  // lanes per sequence in lz4_emit_kernel
constexpr uint64_t kMaxWaves = 4096;      // wavefronts a chunk kernel is launched with at the most: the rest is their grid stride
constexpr uint32_t kScanBlocks = 256;

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

uint64_t boundChunks(uint32_t chunk, uint64_t totalIn, uint64_t nSeg) { return totalIn / chunk + nSeg; }
size_t scratchFor(uint32_t chunk, uint64_t totalIn, uint64_t nSeg) {
    return size_t(lclz4::lz4Layout(nSeg, boundChunks(chunk, totalIn, nSeg), totalIn / 4 + nSeg).bytes);
}

template <bool kMax>
int launchScan(uint8_t* scratch, uint64_t tilesAtMost, hipStream_t st) {
    const uint32_t blocks = uint32_t(std::min<uint64_t>(tilesAtMost ? tilesAtMost : kScanBlocks, kScanBlocks));
    lcNoteKernel("lz4_scan_kernel");
    if (tilesAtMost != 1) {  // (a group of an agent: one launch instead of three)
        hipLaunchKernelGGL(lclz4::lz4_scan_sums_kernel<kMax>, dim3(blocks), dim3(lclz4::kBlock), 0, st, scratch);
        hipLaunchKernelGGL(lclz4::lz4_scan_tiles_kernel<kMax>, dim3(1), dim3(lclz4::kScanTilesPerPass), 0, st, scratch);
    }
    hipLaunchKernelGGL(lclz4::lz4_scan_apply_kernel<kMax>, dim3(blocks), dim3(lclz4::kBlock), 0, st, scratch);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// Everything lc_lz4_compress_device queues.  chunksAtMost: what the host knows of the chunk count (0: nothing) -- it sizes the grids
// only; the kernels take the count from the device.  totalOut: where the emit kernel also leaves the total (a pinned word), or null.
int compressOnStream(const lc_lz4* ctx, const Lz4Job& j, uint8_t* dOut, uint64_t outCap, uint64_t* dOutOff, size_t scratchBytes, uint64_t chunksAtMost,
                     uint64_t* totalOut, hipStream_t st) {
    const uint64_t waves = std::min<uint64_t>(chunksAtMost ? chunksAtMost : kMaxWaves, kMaxWaves);
    const uint64_t tilesAtMost = chunksAtMost ? lclz4::lz4Tiles(chunksAtMost) : 0;
    (void)ctx;
    lcNoteKernel("lz4_plan_kernel");
    hipLaunchKernelGGL(lclz4::lz4_plan_kernel, dim3(1), dim3(lclz4::kPlanBlock), 0, st, j, uint64_t(scratchBytes), dOutOff);
    lcNoteKernel("lz4_match_kernel");
    hipLaunchKernelGGL(lclz4::lz4_match_kernel, dim3(uint32_t((waves + 1) / 2)), dim3(lclz4::kMatchBlock), 0, st, j);
    LC_HIP_TRY(hipGetLastError());
    int rc = launchScan<true>(j.scratch, tilesAtMost, st);
    if (rc != LC_OK) return rc;
    lcNoteKernel("lz4_size_kernel");
    hipLaunchKernelGGL(lclz4::lz4_size_kernel, dim3(uint32_t((waves + 3) / 4)), dim3(lclz4::kBlock), 0, st, j);
    LC_HIP_TRY(hipGetLastError());
    rc = launchScan<false>(j.scratch, tilesAtMost, st);
    if (rc != LC_OK) return rc;
    lcNoteKernel("lz4_emit_kernel");
    hipLaunchKernelGGL(lclz4::lz4_emit_kernel<kEmitLanes>, dim3(uint32_t((waves + 3) / 4)), dim3(lclz4::kBlock), 0, st, j, dOut, outCap, dOutOff, totalOut);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// behind lc_sls_encode_device: the caller's tag bytes right behind the records, the one segment's begin and length, the records' total
// where the host reads it.  Records that did not fit (nothing was stored) leave an empty segment: the host comes back with room.
__global__ void lz4_tags_kernel(const uint64_t* __restrict__ recOff, uint32_t n, uint8_t* __restrict__ rec, uint64_t recCap, const uint8_t* __restrict__ tags,
                                uint32_t tagsLen, uint64_t* __restrict__ segBegin, uint32_t* __restrict__ segLen, uint64_t* __restrict__ rawOut) {
    const uint64_t total = recOff[n];
    const bool fits = total <= recCap && total + tagsLen < lclz4::kLz4SegLimit;
    if (threadIdx.x == 0) {
        *segBegin = 0;
        *segLen = fits ? uint32_t(total + tagsLen) : 0;
        *rawOut = total;
    }
    if (!fits) return;
    for (uint32_t i = threadIdx.x; i < tagsLen; i += blockDim.x) rec[total + i] = tags[i];
}

struct Lz4Thread : TripThread<Lz4Thread> {
    TripBuf hIn, hOut, dIn, dWork, dRec, dScratch;
    Lz4Thread() : TripThread<Lz4Thread>(true) { hIn.pinned = hOut.pinned = true; }
    ~Lz4Thread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dWork, &dRec, &dScratch}); }
};
thread_local Lz4Thread tlsLz4;
constexpr const char* kNoDevice = "no HIP device: the LZ4 block writer has no CPU path";
}  // namespace

extern "C" int lc_lz4_create(uint32_t chunk_bytes, lc_lz4_t** out, char* err, size_t errcap) {
    if (!out) return LC_ERR_ARG;
    *out = nullptr;
    const uint32_t chunk = chunk_bytes ? chunk_bytes : kDefaultChunk;
    if (chunk % 64 || chunk < lclz4::kLz4MinChunk || chunk > lclz4::kLz4MaxChunk) {
        if (err && errcap) std::snprintf(err, errcap, "chunk_bytes %u: a multiple of 64 from 64 to 65536, or 0 for the default", chunk_bytes);
        return LC_ERR_ARG;
    }
    lc_lz4* ctx = new (std::nothrow) lc_lz4{chunk};
    if (!ctx) return LC_ERR_ARG;
    *out = ctx;
    return LC_OK;
}
extern "C" void lc_lz4_free(lc_lz4_t* ctx) { delete ctx; }
extern "C" uint32_t lc_lz4_chunk_bytes(const lc_lz4_t* ctx) { return ctx ? ctx->chunk : 0; }
extern "C" uint64_t lc_lz4_bound(uint64_t n) { return lclz4::lz4Bound(n); }
extern "C" size_t lc_lz4_scratch_bytes(const lc_lz4_t* ctx, uint64_t total_in, uint32_t n_seg) { return ctx ? scratchFor(ctx->chunk, total_in, n_seg) : 0; }

extern "C" int lc_lz4_compress_device(lc_lz4_t* ctx, const uint8_t* d_in, const uint64_t* d_seg_begin, const uint32_t* d_seg_len, uint32_t n_seg,
                                      uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!ctx || !d_out_off || !aligned(d_out_off, 8)) return LC_ERR_ARG;
    if (out_cap && !d_out) return LC_ERR_ARG;
    if (n_seg && (!d_seg_begin || !d_seg_len || !aligned(d_seg_begin, 8) || !aligned(d_seg_len, 4))) return LC_ERR_ARG;
    if (n_seg && (!d_scratch || !aligned(d_scratch, 8) || scratch_bytes < scratchFor(ctx->chunk, 0, n_seg))) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError(kNoDevice);
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(n_seg && d_in ? static_cast<const void*>(d_in) : d_out_off, &dev);  // (never switches devices)
    if (rcDev != LC_OK) return rcDev;
    if (n_seg == 0) {
        LC_HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, static_cast<hipStream_t>(stream)));
        return LC_OK;
    }
    const Lz4Job j{d_in, d_seg_begin, d_seg_len, n_seg, ctx->chunk, static_cast<uint8_t*>(d_scratch)};
    return compressOnStream(ctx, j, d_out, out_cap, d_out_off, scratch_bytes, 0, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" void lc_lz4_thread_release(void) { tlsLz4.release(); }

extern "C" int lc_lz4_compress_host(lc_lz4_t* ctx, const uint8_t* const* segs, const uint32_t* seg_len, uint32_t n_seg, const uint8_t** out,
                                    uint64_t* out_off) {
    if (!ctx || !out || !out_off) return LC_ERR_ARG;
    *out = nullptr;
    out_off[0] = 0;
    if (n_seg && (!segs || !seg_len)) return LC_ERR_ARG;
    uint64_t payload = 0, bound = 0, chunks = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        if (seg_len[s] >= lclz4::kLz4SegLimit || (seg_len[s] && !segs[s])) return LC_ERR_ARG;
        payload += seg_len[s];
        bound += lclz4::lz4Bound(seg_len[s]);
        chunks += lclz4::lz4SegChunks(seg_len[s], ctx->chunk);
    }
    Lz4Thread& T = tlsLz4;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, kNoDevice);
    if (rcBegin != LC_OK) return rcBegin;
    if (n_seg == 0) return LC_OK;
    // up: the segments back to back, their begins, their lengths -- one block, pulled by a kernel
    const size_t beginAt = tripRoundUp(payload + 16, 64), lenAt = beginAt + tripRoundUp(size_t(n_seg) * 8, 64);
    const size_t inBytes = tripRoundUp(lenAt + size_t(n_seg) * 4, 16);
    // down, through the pinned block's mapping: the total, the offsets, the blocks
    const size_t hOffAt = 64, hPayloadAt = hOffAt + tripRoundUp((size_t(n_seg) + 1) * 8, 64);
    const size_t scratchBytes = scratchFor(ctx->chunk, payload, n_seg);
    LC_HIP_TRY(T.hIn.ensure(inBytes));
    LC_HIP_TRY(T.dIn.ensure(inBytes));
    LC_HIP_TRY(T.dScratch.ensure(scratchBytes));
    LC_HIP_TRY(T.hOut.ensure(hPayloadAt + bound));
    uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
    uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
    uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
    uint64_t at = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        reinterpret_cast<uint64_t*>(hIn + beginAt)[s] = at;
        reinterpret_cast<uint32_t*>(hIn + lenAt)[s] = seg_len[s];
        if (seg_len[s]) std::memcpy(hIn + at, segs[s], seg_len[s]);
        at += seg_len[s];
    }
    const Lz4Job j{dIn, reinterpret_cast<const uint64_t*>(dIn + beginAt), reinterpret_cast<const uint32_t*>(dIn + lenAt), n_seg, ctx->chunk,
                   static_cast<uint8_t*>(T.dScratch.p)};
    uint64_t* hTotal = reinterpret_cast<uint64_t*>(hOut);
    int rc = lc_upload_pinned(hIn, dIn, inBytes, T.stream);
    if (rc == LC_OK)
        rc = compressOnStream(ctx, j, hOut + hPayloadAt, T.hOut.cap - hPayloadAt, reinterpret_cast<uint64_t*>(hOut + hOffAt), scratchBytes, chunks, hTotal,
                              T.stream);
    rc = T.end(rc);
    if (rc != LC_OK) return rc;
    if (*hTotal > bound) {
        lcSetLastError("lc_lz4_compress_host: the device refused the batch");
        return LC_ERR_ARG;
    }
    std::memcpy(out_off, hOut + hOffAt, (size_t(n_seg) + 1) * 8);
    *out = hOut + hPayloadAt;
    return LC_OK;
}

extern "C" int lc_lz4_match_encode_compress_host(lc_lz4_t* ctx, lc_sls_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len,
                                                 uint32_t n, const uint32_t* time, const int32_t* time_ns, int enable_ns, const uint8_t* tags,
                                                 uint32_t tags_len, const uint8_t** out, size_t* out_len, uint64_t* raw_len, uint64_t* rec_off,
                                                 uint8_t* status) {
    if (!ctx || !plan || !re || !out || !out_len || !raw_len || (tags_len && !tags)) return LC_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    *raw_len = 0;
    if (tags_len >= lclz4::kLz4SegLimit) return LC_ERR_ARG;
    if (n == 0) {  // no event, no record: the block holds the tags alone
        uint64_t off[2] = {0, 0};
        const int rc = lc_lz4_compress_host(ctx, &tags, &tags_len, 1, out, off);
        if (rc != LC_OK) return rc;
        if (rec_off) rec_off[0] = 0;
        *out_len = size_t(off[1]);
        *raw_len = tags_len;
        return LC_OK;
    }
    if (!lines || !len || !time || !status || n >= (1u << 31)) return LC_ERR_ARG;
    const uint32_t G = uint32_t(lc_regex_mark_count(re));
    if (plan->maxSource > G) return LC_ERR_ARG;
    Lz4Thread& T = tlsLz4;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, kNoDevice);
    if (rcBegin != LC_OK) return rcBegin;
    uint64_t payload = 0;
    for (uint32_t i = 0; i < n; ++i) payload += len[i];
    if (payload >= (1ull << 31)) {
        lcSetLastError("lc_lz4_match_encode_compress_host: 2 GiB of lines or more in one call");
        return LC_ERR_ARG;
    }
    // up: the lines back to back, their n + 1 offsets, the times, the nanosecond parts, the tags -- one block, pulled by a kernel
    const bool ns = enable_ns && time_ns;
    const size_t offAt = tripOffAt(payload), timeAt = offAt + tripRoundUp((size_t(n) + 1) * 4, 16), nsAt = timeAt + tripRoundUp(size_t(n) * 4, 16);
    const size_t tagsAt = tripRoundUp(nsAt + (ns ? size_t(n) * 4 : 0), 16), inBytes = tripRoundUp(tagsAt + tags_len, 16);
    // on the device: rows, record offsets, the record scan's scratch, the one segment's begin and length
    const size_t recOffAt = tripRoundUp(size_t(n) * 2 * G * 4, 16), slsScratchAt = recOffAt + tripRoundUp((size_t(n) + 1) * 8, 16);
    const size_t slsScratchBytes = lc_sls_scratch_bytes(n), segAt = slsScratchAt + tripRoundUp(slsScratchBytes, 16);
    // down, through the pinned block's mapping: the block's size, the records' size, the block's offsets, the status bytes, the block
    const size_t hRawAt = 8, hOffAt = 16, hStatusAt = 64, hPayloadAt = hStatusAt + tripRoundUp(n, 64);
    // what the records take when no line's rows overlap: the room the first attempt gets (lc_sls_match_encode_host's rule)
    const uint64_t fixed = std::max(plan->boundFixed[0], plan->boundFixed[1]), perLine = std::max(plan->boundLines[0], plan->boundLines[1]);
    uint64_t recCap = tripRoundUp(uint64_t(n) * fixed + perLine * payload, 16);
    LC_HIP_TRY(T.hIn.ensure(inBytes));
    LC_HIP_TRY(T.dIn.ensure(inBytes));
    LC_HIP_TRY(T.dWork.ensure(segAt + 16));
    uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
    uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
    uint8_t* dWork = static_cast<uint8_t*>(T.dWork.p);
    tripPackLines(hIn, offAt, lines, len, 0, n);
    reinterpret_cast<uint32_t*>(hIn + offAt)[n] = uint32_t(payload);
    std::memcpy(hIn + timeAt, time, size_t(n) * 4);
    if (ns) std::memcpy(hIn + nsAt, time_ns, size_t(n) * 4);
    if (tags_len) std::memcpy(hIn + tagsAt, tags, tags_len);
    const uint32_t* dOff = reinterpret_cast<const uint32_t*>(dIn + offAt);
    uint64_t* dRecOff = reinterpret_cast<uint64_t*>(dWork + recOffAt);
    uint64_t* dSegBegin = reinterpret_cast<uint64_t*>(dWork + segAt);
    uint32_t* dSegLen = reinterpret_cast<uint32_t*>(dWork + segAt + 8);
    uint64_t total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const uint64_t rawCap = recCap + tags_len;
        if (rawCap >= lclz4::kLz4SegLimit) {
            lcSetLastError("lc_lz4_match_encode_compress_host: the group's records reach the segment limit");
            return LC_ERR_ARG;
        }
        const size_t scratchBytes = scratchFor(ctx->chunk, rawCap, 1);
        LC_HIP_TRY(T.dRec.ensure(rawCap + 16));
        LC_HIP_TRY(T.dScratch.ensure(scratchBytes));
        LC_HIP_TRY(T.hOut.ensure(hPayloadAt + lclz4::lz4Bound(rawCap)));
        uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
        uint8_t* dRec = static_cast<uint8_t*>(T.dRec.p);
        if (attempt) std::memcpy(hOut + hStatusAt, status, n);  // (the pinned block moved: the status bytes are with the caller already)
        int rc = LC_OK;
        if (!attempt) {
            rc = lc_upload_pinned(hIn, dIn, inBytes, T.stream);
            if (rc == LC_OK) rc = lc_regex_match_device(re, dIn, dOff, nullptr, 0, n, G, reinterpret_cast<int32_t*>(dWork), hOut + hStatusAt, T.stream);
        }
        if (rc == LC_OK)
            rc = lc_sls_encode_device(plan, dIn, dOff, nullptr, 0, n, G, reinterpret_cast<const int32_t*>(dWork), hOut + hStatusAt,
                                      reinterpret_cast<const uint32_t*>(dIn + timeAt), ns ? reinterpret_cast<const int32_t*>(dIn + nsAt) : nullptr, ns ? 1 : 0,
                                      dRec, recCap, dRecOff, dWork + slsScratchAt, slsScratchBytes, T.stream);
        if (rc == LC_OK) {
            lcNoteKernel("lz4_tags_kernel");
            hipLaunchKernelGGL(lz4_tags_kernel, dim3(1), dim3(256), 0, T.stream, dRecOff, n, dRec, recCap, dIn + tagsAt, tags_len, dSegBegin, dSegLen,
                               reinterpret_cast<uint64_t*>(hOut + hRawAt));
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) rc = lcHipFail(e, "lz4_tags_kernel");
        }
        const Lz4Job j{dRec, dSegBegin, dSegLen, 1, ctx->chunk, static_cast<uint8_t*>(T.dScratch.p)};
        if (rc == LC_OK)
            rc = compressOnStream(ctx, j, hOut + hPayloadAt, T.hOut.cap - hPayloadAt, reinterpret_cast<uint64_t*>(hOut + hOffAt), scratchBytes,
                                  boundChunks(ctx->chunk, rawCap, 1), reinterpret_cast<uint64_t*>(hOut), T.stream);
        if (rc == LC_OK && rec_off) {  // (only a caller that asks for the offsets pays a copy)
            const hipError_t e = hipMemcpyAsync(rec_off, dRecOff, (size_t(n) + 1) * 8, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(SLS record offsets)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        total = *reinterpret_cast<const uint64_t*>(hOut + hRawAt);
        if (!attempt) std::memcpy(status, hOut + hStatusAt, n);
        if (total <= recCap) {
            const uint64_t block = *reinterpret_cast<const uint64_t*>(hOut);
            if (block > lclz4::lz4Bound(total + tags_len)) {
                lcSetLastError("lc_lz4_match_encode_compress_host: the device refused the group");
                return LC_ERR_ARG;
            }
            *out = hOut + hPayloadAt;
            *out_len = size_t(block);
            *raw_len = total + tags_len;
            return LC_OK;
        }
        // rows that overlap (nested groups, the line beside its groups): the records once more, into a buffer with room for all of them
        recCap = tripRoundUp(total, 16);
    }
    lcSetLastError("lc_lz4_match_encode_compress_host: the records grew between two attempts");
    return LC_ERR_HIP;
}
