// json_kernel.hpp -- json_walk_kernel: the JSON parser's walk on gfx950 (wave64), included by json_device.hip only.
//
// One line per lane, jsonWalkLine() of json_vm.hpp per lane, over the staged wavefront tile of wave_tile_source.hpp (the source
// delim_split_kernel reads through: aligned 16-byte global loads inside the line's own 16-byte units, swizzled ds_read_b128, the next
// stage in flight while this one is walked).  Results are written by the line's own lane with plain vector stores: a status byte, the
// member count, the error offset, up to W records of 20 bytes, and the unescaped bytes of escaped top-level texts into the shadow
// buffer at the text's own offset.  No atomics, no table: character classes are compares, the nesting stack is two registers.
//
// DEEP = true is the second launch: it looks only at lines whose status is LC_JSON_DEEP (nested deeper than 64 levels), walks them
// again from their first byte with the nesting stack in a per-lane slice of device scratch (32 words: 1024 levels), and overwrites
// their results.  Its grid is fixed (kDeepBlocks), so the scratch is; a wavefront without such a line moves on at once.
#pragma once

#include <hip/hip_runtime.h>

#include "json_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcjsonk {

constexpr int kBlock = 256;
constexpr uint32_t kDeepBlocks = 64;
constexpr size_t kDeepScratchBytes = size_t(kDeepBlocks) * kBlock * kJsonDeepWords * 4;
static_assert(kJsonStageBytes == lcwave::kWaveStageBytes, "jsonWalkLine walks the stages WaveTileSource hands out");

template <bool DEEP>
__global__ __launch_bounds__(kBlock) void json_walk_kernel(const uint8_t* __restrict__ data, const int32_t* __restrict__ off, uint32_t n,
                                                           uint32_t W, uint8_t* __restrict__ status, uint32_t* __restrict__ nmembers,
                                                           uint32_t* __restrict__ errpos, lc_json_member_t* __restrict__ records,
                                                           uint8_t* __restrict__ shadow, uint32_t* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * lcwave::kWaveTileBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * lcwave::kWaveTileBytes;  // LDS byte address
    uint32_t* deep = DEEP ? scratch + (size_t(blockIdx.x) * kBlock + tid) * kJsonDeepWords : nullptr;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t line = base + tid;
        bool live = line < n;
        if (DEEP) {
            live = live && status[line] == LC_JSON_DEEP;
            if (!__any(live)) continue;  // (wavefront-uniform: the cooperative stages below never cross a wavefront)
        }
        uint32_t o = 0, len = 0;
        if (live) {
            o = uint32_t(off[line]);
            len = uint32_t(off[line + 1]) - o;
        }
        lcwave::WaveTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + o);
        uint8_t st = LC_JSON_FAIL;
        uint32_t count = 0, err = 0;
        lc_json_member_t* row = records + size_t(live ? line : 0u) * W;
        // (a lane without a line walks a line of length 0: it takes part in the cooperative stages and writes nothing)
        jsonWalkLine<DEEP>(src, len, live ? W : 0u, row, shadow + o, deep, &st, &count, &err);
        if (live) {
            status[line] = st;
            nmembers[line] = count;
            errpos[line] = err;
        }
        if (!DEEP) break;  // (the first launch has one block per 256 lines)
    }
}

}  // namespace lcjsonk
