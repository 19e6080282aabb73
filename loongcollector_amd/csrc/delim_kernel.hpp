// delim_kernel.hpp -- delim_split_kernel: the delimiter parser's split on gfx950 (wave64), included by delim_device.hip only.
//
// One line per lane, delimSplitLine() of delim_vm.hpp per lane; this file is only the SOURCE that routine reads through:
//   * a wavefront owns a tile of 64 rows x 64 bytes in LDS (4 KB; 16 KB per 256-thread workgroup).  A row is one line's current
//     64-byte stage, counted from the 16-byte boundary at or below the line's first byte, so every global access is an ALIGNED
//     16-byte load (global_load_dwordx4) that stays inside the line's own 16-byte units -- the contract of lc_regex_gpu.h for d_data.
//   * a stage is fetched by the whole wavefront: four loads per lane, lanes 4r .. 4r+3 fetch the four quads of row r (+16 rows per
//     load), so the four lanes of a row read 64 consecutive bytes.  Stage s + 1 is in flight (in registers) while the lanes walk
//     stage s; each byte of a line is fetched once by this loop.  The trim of trailing blanks looks at the line's last quad before
//     the walk (one more 16-byte load per line, of a cache line the stage loop fetches anyway).
//   * a lane reads ITS row as four ds_read_b128; the 16-byte segments of a row are XOR-swizzled by (row >> 1) & 3 so that the 64
//     lanes' reads of "their segment k" spread over all banks (rows are 64 bytes apart: unswizzled, lanes 0, 2, 4 ... would meet).
//   * results: one status byte, one count and up to W (begin, end) pairs per line, written by the line's lane as it finds them
//     (global_store_dwordx2).  No atomics, no table: the four states live in a register.
// The stage loop's trip count is the wavefront's longest line; a lane whose line has ended (or failed) idles through the rest.
#pragma once

#include <hip/hip_runtime.h>

#include "delim_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcdelim {

constexpr int kBlock = 256;
static_assert(kDelimStageBytes == lcwave::kWaveStageBytes, "delimSplitLine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront
using lcwave::WaveTileSource;

template <bool QUOTE>
__global__ __launch_bounds__(kBlock) void delim_split_kernel(DelimConfig cfg, const uint8_t* __restrict__ data,
                                                             const int32_t* __restrict__ off, uint32_t n, uint32_t W,
                                                             uint8_t* __restrict__ status, uint32_t* __restrict__ ncols,
                                                             int32_t* __restrict__ spans) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t line = blockIdx.x * kBlock + tid;
    const bool live = line < n;
    uint32_t o = 0, len = 0;
    if (live) {
        o = uint32_t(off[line]);
        len = uint32_t(off[line + 1]) - o;
    }
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * kTileBytes;  // LDS byte address
    WaveTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + o);
    uint8_t st = LC_DELIM_FAIL;
    uint32_t count = 0;
    DelimSpan* row = reinterpret_cast<DelimSpan*>(spans) + size_t(live ? line : 0u) * W;
    // (a lane without a line walks a line of length 0: it takes part in the cooperative stages and writes nothing -- W = 0 for it)
    delimSplitLine<QUOTE>(cfg, src, len, live ? W : 0u, row, &st, &count);
    if (live) {
        status[line] = st;
        ncols[line] = count;
    }
}

}  // namespace lcdelim
