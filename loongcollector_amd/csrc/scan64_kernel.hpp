// scan64_kernel.hpp -- the 64-bit exclusive scan of a device array in place, as one header: tile sums, one workgroup over the sums,
// tile scan (the three launches desens_kernel.hpp, sls_kernel.hpp and lz4_kernel.hpp each restate; those copies stay as they are).
// An array of one tile takes the last launch alone.  The caller hands m values and lcscan::tileSumBytes(m) bytes of scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lcscan {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWavesPerBlock = kBlock / 64;
constexpr uint32_t kPerThread = 4;
constexpr uint32_t kTile = kBlock * kPerThread;
constexpr uint32_t kTilesPerPass = 1024;

inline uint32_t tiles(uint64_t m) { return uint32_t((m + kTile - 1) / kTile); }
inline size_t tileSumBytes(uint64_t m) { return size_t(tiles(m)) * 8; }

__device__ __forceinline__ uint64_t waveInclusive(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= uint32_t(d)) v += up;
    }
    return v;
}

static __global__ __launch_bounds__(kBlock) void scan64_sums_kernel(const uint64_t* __restrict__ values, uint32_t m, uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint64_t base = uint64_t(blockIdx.x) * kTile + threadIdx.x * kPerThread;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPerThread; ++q)
        if (base + q < m) v += values[base + q];
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

// exclusive scan of tileSums[0..nTiles) in place.  One workgroup of kTilesPerPass lanes, one pass per kTilesPerPass tiles.
static __global__ __launch_bounds__(kTilesPerPass) void scan64_tiles_kernel(uint64_t* __restrict__ tileSums, uint32_t nTiles) {
    __shared__ uint64_t waveSums[kTilesPerPass / 64];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nTiles; base += kTilesPerPass) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nTiles ? tileSums[i] : 0;
        const uint64_t incl = waveInclusive(v, lane);
        if (lane == 63) waveSums[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += waveSums[w];
        if (i < nTiles) tileSums[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kTilesPerPass - 1) carry = before + incl;
        __syncthreads();
    }
}

static __global__ __launch_bounds__(kBlock) void scan64_apply_kernel(uint64_t* __restrict__ values, uint32_t m, const uint64_t* __restrict__ tileSums) {
    __shared__ uint64_t waveSums[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = uint64_t(blockIdx.x) * kTile + threadIdx.x * kPerThread;
    uint64_t own[kPerThread];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPerThread; ++q) {
        own[q] = base + q < m ? values[base + q] : 0;
        sum += own[q];
    }
    const uint64_t incl = waveInclusive(sum, lane);
    if (lane == 63) waveSums[wave] = incl;
    __syncthreads();
    uint64_t at = (tileSums ? tileSums[blockIdx.x] : 0) + incl - sum;  // (no tile sums: the array is one tile)
    for (uint32_t w = 0; w < wave; ++w) at += waveSums[w];
#pragma unroll
    for (uint32_t q = 0; q < kPerThread; ++q) {
        if (base + q < m) values[base + q] = at;
        at += own[q];
    }
}

// values[0..m) becomes its exclusive scan (m >= 1, m <= 2^31); tileSums: tileSumBytes(m) bytes, 8-byte aligned
inline hipError_t exclusiveScan(uint64_t* values, uint32_t m, uint64_t* tileSums, hipStream_t st) {
    const uint32_t t = tiles(m);
    if (t == 1) {
        hipLaunchKernelGGL(scan64_apply_kernel, dim3(1), dim3(kBlock), 0, st, values, m, static_cast<const uint64_t*>(nullptr));
    } else {
        hipLaunchKernelGGL(scan64_sums_kernel, dim3(t), dim3(kBlock), 0, st, values, m, tileSums);
        hipLaunchKernelGGL(scan64_tiles_kernel, dim3(1), dim3(kTilesPerPass), 0, st, tileSums, t);
        hipLaunchKernelGGL(scan64_apply_kernel, dim3(t), dim3(kBlock), 0, st, values, m, static_cast<const uint64_t*>(tileSums));
    }
    return hipGetLastError();
}

}  // namespace lcscan
