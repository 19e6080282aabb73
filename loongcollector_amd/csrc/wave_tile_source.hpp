// wave_tile_source.hpp -- the SOURCE the one-line-per-lane kernels read through (delim_kernel.hpp, json_kernel.hpp), gfx950, wave64:
//   * a wavefront owns a tile of 64 rows x 64 bytes in LDS (4 KB; 16 KB per 256-thread workgroup).  A row is one line's current
//     64-byte stage, counted from the 16-byte boundary at or below the line's first byte, so every global access is an ALIGNED
//     16-byte load (global_load_dwordx4) that stays inside the line's own 16-byte units -- the contract of lc_regex_gpu.h for d_data.
//   * a stage is fetched by the whole wavefront: four loads per lane, lanes 4r .. 4r+3 fetch the four quads of row r (+16 rows per
//     load), so the four lanes of a row read 64 consecutive bytes.  Stage s + 1 is in flight (in registers) while the lanes walk
//     stage s; each byte of a line is fetched once by this loop.
//   * a lane reads ITS row as four ds_read_b128; the 16-byte segments of a row are XOR-swizzled by (row >> 1) & 3 so that the 64
//     lanes' reads of "their segment k" spread over all banks (rows are 64 bytes apart: unswizzled, lanes 0, 2, 4 ... would meet).
// The stage loop's trip count is the wavefront's longest line; a lane whose line has ended (or failed) idles through the rest.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lcwave {

constexpr uint32_t kWaveStageBytes = 64;
constexpr uint32_t kWaveTileBytes = 64 * kWaveStageBytes;  // per wavefront

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((address_space(3))) * LdsQuadPtr;
typedef const u32x4 __attribute__((address_space(1))) * GlobalQuadPtr;

__device__ __forceinline__ void waveLdsSync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct WaveTileSource {
    uint32_t lane, tile;       // tile: LDS byte address of the wavefront's tile
    uint32_t headBytes;
    uintptr_t rowStart;        // global address of this lane's row (16-byte aligned)
    uint32_t myRow, mySwizzle;
    uintptr_t srcRow[4];       // row starts of the rows this lane fetches for
    uint32_t srcEnd[4], dstAddr[4], seg;
    u32x4 in[4];

    __device__ __forceinline__ WaveTileSource(uint32_t lane_, uint32_t tile_, uintptr_t lineAddr)
        : lane(lane_), tile(tile_), headBytes(uint32_t(lineAddr & 15u)), rowStart(lineAddr - (lineAddr & 15u)) {
        myRow = tile + lane * kWaveStageBytes;
        mySwizzle = ((lane >> 1) & 3u) << 4;
        seg = (lane & 3u) * 16;
    }
    __device__ __forceinline__ uint32_t head() const { return headBytes; }
    __device__ __forceinline__ void tailQuad(uint32_t p16, uint32_t q[4]) const {
        const u32x4 v = *reinterpret_cast<GlobalQuadPtr>(rowStart + p16);
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    }
    // one byte of the line at tile position p (head <= p < the line's end), straight from memory: for the rare re-read
    __device__ __forceinline__ uint32_t byteAt(uint32_t p) const { return *reinterpret_cast<const uint8_t*>(rowStart + p); }
    __device__ __forceinline__ void fetch(uint32_t s) {  // stage s -> in[]
        const uint32_t at = s * kWaveStageBytes + seg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            in[i] = u32x4{0, 0, 0, 0};
            if (at < srcEnd[i]) in[i] = *reinterpret_cast<GlobalQuadPtr>(srcRow[i] + at);
        }
    }
    // end: this lane's trimmed end in tile coordinates (0: nothing to walk).  Every lane of the wavefront calls this together.
    __device__ __forceinline__ uint32_t stageCount(uint32_t end) {
        uint32_t stages = (end + kWaveStageBytes - 1) / kWaveStageBytes;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t other = __shfl_xor(stages, d, 64);
            stages = other > stages ? other : stages;
        }
        stages = __builtin_amdgcn_readfirstlane(stages);
        const uint32_t lo = uint32_t(rowStart), hi = uint32_t(uint64_t(rowStart) >> 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * i + int(lane >> 2);
            srcRow[i] = uintptr_t((uint64_t(__shfl(hi, r, 64)) << 32) | __shfl(lo, r, 64));
            srcEnd[i] = __shfl(end, r, 64);
            dstAddr[i] = tile + uint32_t(r) * kWaveStageBytes + (seg ^ (((uint32_t(r) >> 1) & 3u) << 4));
        }
        if (stages) fetch(0);
        return stages;
    }
    __device__ __forceinline__ void stage(uint32_t s) {
        waveLdsSync();  // every lane has read its row of the stage before
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<LdsQuadPtr>(dstAddr[i]) = in[i];
        waveLdsSync();
        fetch(s + 1);  // (past the longest line: no lane's guard passes, nothing is issued)
    }
    __device__ __forceinline__ void rowQuad(uint32_t k, uint32_t q[4]) const {
        const u32x4 v = *reinterpret_cast<LdsQuadPtr>(myRow + ((k * 16) ^ mySwizzle));
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    }
};

}  // namespace lcwave
