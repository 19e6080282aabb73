// desens_kernel.hpp -- the gfx950 kernels of processor_desensitize_gpu (launched by desens_device.hip; the per-value rules are
// desens_vm.hpp's, shared with the host):
//   desens_init_kernel     per value: its length, the search state, round 0's list
//   desens_collect_kernel  after each search round, one lane per value of the round's list: the method's rule on the engine's row -- a cut
//                          appended to the value's chain, a byte stepped over, the value marked unchanged, or finished; the resume offset
//                          (`const`) or the private offset / length copy (`md5`) advanced; the next round's list and its device-side count
//   desens_size_kernel     per value: the output length from its chain (0 for an unchanged value) and the value's flags
//   desens_scan_*          the 64-bit exclusive scan of the lengths into out_off[n + 1] (tile sums, one workgroup over the sums in the
//                          way of split_scan_kernel, tile scan)
//   desens_write_kernel    a wavefront per changed value: every copy strided over the 64 lanes (a wave instruction reads and writes 64
//                          consecutive bytes), digests one lane per cut
// Plain C++ stores only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "desens_vm.hpp"

namespace lcdesens {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWavesPerBlock = kBlock / 64;
constexpr uint32_t kScanPerThread = 4;
constexpr uint32_t kScanTile = kBlock * kScanPerThread;

// what the kernels share about a batch; every array is indexed by value
struct Batch {
    const uint8_t* data;
    const uint32_t* off;
    uint32_t* len;      // the values' lengths (computed from off when the caller gave none)
    uint32_t* from;     // ValueState, as arrays
    uint32_t* lastEnd;
    uint32_t* last;
    uint8_t* vflags;
    uint32_t* offP;     // md5: the suffix the next search sees
    uint32_t* lenP;
    uint32_t n;
};

__global__ __launch_bounds__(kBlock) void desens_init_kernel(Batch b, const uint32_t* __restrict__ lenIn, bool md5, uint32_t* __restrict__ list) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= b.n) return;
    const uint32_t len = lenIn ? lenIn[i] : b.off[i + 1] - b.off[i];
    b.len[i] = len;
    b.from[i] = 0;
    b.lastEnd[i] = kNone;
    b.last[i] = kNone;
    b.vflags[i] = 0;
    if (md5) {
        b.offP[i] = b.off[i];
        b.lenP[i] = len;
    }
    list[i] = i;
}

// count: how many entries of `list` this round searched (the host knows it: it read the word the last round left).  recs + recBase: this
// round's `count` record slots.  *countOut was zeroed on the stream.
__global__ __launch_bounds__(kBlock) void desens_collect_kernel(Batch b, Program P, const uint32_t* __restrict__ refGroup, bool replacingAll,
                                                                const uint32_t* __restrict__ list, uint32_t count,
                                                                const int32_t* __restrict__ caps, uint32_t capsPerValue,
                                                                const uint8_t* __restrict__ status, uint32_t* __restrict__ recs, uint32_t recBase,
                                                                uint32_t* __restrict__ listOut, uint32_t* __restrict__ countOut) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    bool again = false;
    uint32_t v = 0;
    if (k < count) {
        v = list[k];
        ValueState S{b.from[v], b.lastEnd[v], b.last[v]};
        uint8_t flags = b.vflags[v];
        const uint32_t n = b.len[v];
        const uint32_t recIdx = recBase + k;
        again = collectStep(P, refGroup, replacingAll, n, status[v], caps + size_t(v) * capsPerValue, S, recIdx, recs + size_t(recIdx) * recWords(P),
                            flags);
        b.from[v] = S.from;
        b.lastEnd[v] = S.lastEnd;
        b.last[v] = S.last;
        b.vflags[v] = flags;
        if (again && P.method == kMethodMd5) {
            b.offP[v] = b.off[v] + S.from;
            b.lenP[v] = n - S.from;
        }
    }
    // the next round's list: one atomic per wavefront
    const uint64_t mask = __ballot(again);
    if (mask == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    uint32_t base = 0;
    if (int(lane) == leader) base = atomicAdd(countOut, uint32_t(__popcll(mask)));
    base = __shfl(base, leader, 64);
    if (again) listOut[base + uint32_t(__popcll(mask & ((1ull << lane) - 1)))] = v;
}

__global__ __launch_bounds__(kBlock) void desens_size_kernel(Batch b, Program P, const uint32_t* __restrict__ recs, uint8_t* __restrict__ flags,
                                                             uint64_t* __restrict__ sizes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > b.n) return;
    if (i == b.n) {  // the scan's last element: out_off[n] becomes the total
        sizes[i] = 0;
        return;
    }
    const uint32_t last = b.last[i];
    const bool changed = last != kNone;
    sizes[i] = changed ? outLen(P, b.len[i], last, recs) : 0;
    flags[i] = uint8_t((changed ? kFlagChanged : 0) | (b.vflags[i] & kFlagGaveUp));
}

// ---- exclusive scan of sizes[0..m) in place, 64-bit
__device__ __forceinline__ uint64_t waveInclusive(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= uint32_t(d)) v += up;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void desens_scan_sums_kernel(const uint64_t* __restrict__ sizes, uint32_t m, uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanPerThread;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScanPerThread; ++q)
        if (base + q < m) v += sizes[base + q];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
    if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0;
        for (uint32_t w = 0; w < kWavesPerBlock; ++w) total += waveSums[w];
        tileSums[blockIdx.x] = total;
    }
}

// exclusive scan of tileSums[0..nTiles) in place.  One workgroup of 1024 lanes.
__global__ __launch_bounds__(1024) void desens_scan_tiles_kernel(uint64_t* __restrict__ tileSums, uint32_t nTiles) {
    __shared__ uint64_t waveSums[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nTiles; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nTiles ? tileSums[i] : 0;
        const uint64_t incl = waveInclusive(v, lane);
        if (lane == 63) waveSums[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += waveSums[w];
        if (i < nTiles) tileSums[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void desens_scan_apply_kernel(uint64_t* __restrict__ sizes, uint32_t m, const uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanPerThread;
    uint64_t own[kScanPerThread];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScanPerThread; ++q) {
        own[q] = base + q < m ? sizes[base + q] : 0;
        sum += own[q];
    }
    const uint64_t incl = waveInclusive(sum, lane);
    if (lane == 63) waveSums[wave] = incl;
    __syncthreads();
    uint64_t at = tileSums[blockIdx.x] + incl - sum;
    for (uint32_t w = 0; w < wave; ++w) at += waveSums[w];
#pragma unroll
    for (uint32_t q = 0; q < kScanPerThread; ++q) {
        if (base + q < m) sizes[base + q] = at;
        at += own[q];
    }
}

// a wavefront per value; out: the trip's output bytes, outOff[i] where value i's begin
__global__ __launch_bounds__(kBlock) void desens_write_kernel(Batch b, Program P, const uint32_t* __restrict__ recs, const uint64_t* __restrict__ outOff,
                                                              uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= b.n) return;
    const uint32_t last = b.last[i];
    if (last == kNone) return;
    const uint64_t at = outOff[i];
    writeValue(P, b.data + b.off[i], b.len[i], out + at, uint32_t(outOff[i + 1] - at), last, recs, threadIdx.x & 63, 64);
}

}  // namespace lcdesens
