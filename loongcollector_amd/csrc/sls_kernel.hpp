// sls_kernel.hpp -- the gfx950 kernels of the SLS encoder (launched by sls_device.hip; the per-event rules are sls_vm.hpp's, shared
// with the host):
//   sls_size_kernel    one lane per event: the status byte, the capture row and the line length -> the record's size (0: no record)
//   sls_scan_*         the 64-bit exclusive scan of the sizes into rec_off[n + 1], rec_off[n] the total (tile sums, one workgroup over
//                      the sums, tile scan: the three launches of desens_kernel.hpp, restated; a batch of one tile takes the last alone)
//   sls_write_kernel   kLanes lanes per event; a lane owns ALIGNED dwords of the output and assembles each from the pieces that cover
//                      it (slsRecordWord): every word inside a record is one 4-byte store, consecutive lanes store consecutive words;
//                      only a record's first and last partial word are byte stores.  Nothing is stored when the total exceeds out_cap.
// Plain C++ stores only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sls_vm.hpp"

namespace lcsls {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWavesPerBlock = kBlock / 64;
constexpr uint32_t kScanPerThread = 4;
constexpr uint32_t kScanTile = kBlock * kScanPerThread;
constexpr uint32_t kScanTilesPerPass = 1024;

// what lc_regex_match_device left behind, and the events' times
struct SlsBatch {
    const uint8_t* data;
    const uint32_t* off;
    const uint32_t* len;  // may be null: len[i] = off[i + 1] - off[i] - sep
    uint32_t sep, n, ngroups;
    const int32_t* caps;
    const uint8_t* status;
    const uint32_t* time;
    const int32_t* timeNs;  // may be null; < 0: none
    uint32_t enableNs;
};

__device__ __forceinline__ SlsEvent loadEvent(const SlsPlanView& P, const SlsBatch& b, uint32_t i) {
    SlsEvent e;
    const uint32_t at = b.off[i];
    if (b.len) {
        e.lineLen = b.len[i];
    } else {
        const uint32_t span = b.off[i + 1] - at;
        e.lineLen = span >= b.sep ? span - b.sep : 0;
    }
    e.line = b.data + at;
    e.caps = b.caps + size_t(i) * 2 * b.ngroups;
    eventItems(P, b.status[i], &e.firstItem, &e.nItems);
    e.time = b.time[i];
    const int32_t ns = (b.enableNs && b.timeNs) ? b.timeNs[i] : -1;
    e.hasNs = ns >= 0;
    e.ns = uint32_t(ns);
    return e;
}

__global__ __launch_bounds__(kBlock) void sls_size_kernel(SlsPlanView P, SlsBatch b, uint64_t* __restrict__ sizes) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > b.n) return;
    if (i == b.n) {  // the scan's last element: rec_off[n] becomes the total
        sizes[i] = 0;
        return;
    }
    sizes[i] = slsRecordSize(P, loadEvent(P, b, i));
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

__global__ __launch_bounds__(kBlock) void sls_scan_sums_kernel(const uint64_t* __restrict__ sizes, uint32_t m, uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + threadIdx.x * kScanPerThread;
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

// exclusive scan of tileSums[0..nTiles) in place.  One workgroup of kScanTilesPerPass lanes, one pass per kScanTilesPerPass tiles.
__global__ __launch_bounds__(kScanTilesPerPass) void sls_scan_tiles_kernel(uint64_t* __restrict__ tileSums, uint32_t nTiles) {
    __shared__ uint64_t waveSums[kScanTilesPerPass / 64];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nTiles; base += kScanTilesPerPass) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nTiles ? tileSums[i] : 0;
        const uint64_t incl = waveInclusive(v, lane);
        if (lane == 63) waveSums[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += waveSums[w];
        if (i < nTiles) tileSums[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kScanTilesPerPass - 1) carry = before + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void sls_scan_apply_kernel(uint64_t* __restrict__ sizes, uint32_t m, const uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + threadIdx.x * kScanPerThread;
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
    uint64_t at = (tileSums ? tileSums[blockIdx.x] : 0) + incl - sum;  // (no tile sums: the batch is one tile)
    for (uint32_t w = 0; w < wave; ++w) at += waveSums[w];
#pragma unroll
    for (uint32_t q = 0; q < kScanPerThread; ++q) {
        if (base + q < m) sizes[base + q] = at;
        at += own[q];
    }
}

// kLanes lanes per event (a divisor of 64); out is 16-byte aligned, so an aligned word of a record is an aligned word of memory
template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void sls_write_kernel(SlsPlanView P, SlsBatch b, const uint64_t* __restrict__ recOff, uint8_t* __restrict__ out,
                                                           uint64_t outCap, uint64_t* __restrict__ totalOut) {
    // (the host entry's trip: the total goes where the host reads it, through the pinned mapping)
    if (totalOut && blockIdx.x == 0 && threadIdx.x == 0) *totalOut = recOff[b.n];
    if (recOff[b.n] > outCap) return;  // too small: not one byte is stored
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    if (i64 >= b.n) return;
    const uint32_t i = uint32_t(i64);
    const uint64_t at = recOff[i];
    const uint32_t size = uint32_t(recOff[i + 1] - at);
    if (size == 0) return;
    const SlsEvent e = loadEvent(P, b, i);
    const uint32_t lead = uint32_t(at & 3u);
    uint8_t* base = out + (at - lead);
    const uint32_t end = lead + size;
    SlsCursor c = slsCursorBegin(P, e, lead, size);
    for (uint64_t q64 = uint64_t(threadIdx.x % kLanes) * 4; q64 < end; q64 += uint64_t(kLanes) * 4) {
        const uint32_t q = uint32_t(q64);
        const uint32_t w = slsRecordWord(P, e, c, q);
        if (q >= lead && q + 4 <= end) {
            *reinterpret_cast<uint32_t*>(base + q) = w;
        } else {  // the record's first or last partial word: its neighbours own the other bytes
            for (uint32_t j = 0; j < 4; ++j)
                if (q + j >= lead && q + j < end) base[q + j] = uint8_t(w >> (8 * j));
        }
    }
}

}  // namespace lcsls
