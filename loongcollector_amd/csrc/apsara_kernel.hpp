// apsara_kernel.hpp -- apsara_parse_kernel: the Apsara parser's per-line work on gfx950 (wave64), included by apsara_device.hip only.
//
// One line per lane, apsaraParseLine() of apsara_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of
// 64 rows x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one line's current 64-byte stage, fetched by the whole wavefront
// as aligned 16-byte loads inside the line's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.  Each byte of a
// line is fetched once by that loop.  The time text lies in stage 0 (a '[' at tile position <= 15 and some thirty bytes), so the time
// routine runs while stage 0 is current and reads its bytes from the lane's LDS row (ds_read_u8); only a time text that runs past
// tile byte 63 -- a long run of blanks, a long row of digits -- reads those bytes again, from memory (byteAt).
// Results: per line one status byte, seconds, nanoseconds, four (begin, end) base-field spans, the TRUE pair count and up to W
// (key begin, colon, end) triples, all written by the line's own lane as plain vector stores.  No atomics.
#pragma once

#include <hip/hip_runtime.h>

#include "apsara_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcapsara {

constexpr int kBlock = 256;
static_assert(kApsaraStageBytes == lcwave::kWaveStageBytes, "apsaraParseLine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront

struct ApsaraTileSource : lcwave::WaveTileSource {
    using lcwave::WaveTileSource::WaveTileSource;
    typedef const uint8_t __attribute__((address_space(3))) * LdsBytePtr;
    // head < p < the line's end; stage 0 is current
    __device__ __forceinline__ uint32_t timeByte(uint32_t p) const {
        if (p < lcwave::kWaveStageBytes) return *reinterpret_cast<LdsBytePtr>(myRow + (((p & ~15u) ^ mySwizzle) | (p & 15u)));
        return byteAt(p);
    }
};

__global__ __launch_bounds__(kBlock) void apsara_parse_kernel(const uint8_t* __restrict__ data, const int32_t* __restrict__ off, uint32_t n,
                                                              uint32_t W, uint8_t* __restrict__ status, int64_t* __restrict__ secs,
                                                              uint32_t* __restrict__ nanos, int32_t* __restrict__ base,
                                                              uint32_t* __restrict__ npairs, int32_t* __restrict__ pairs) {
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
    ApsaraTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + o);
    ApsaraPair* row = reinterpret_cast<ApsaraPair*>(pairs) + size_t(live ? line : 0u) * W;
    ApsaraLine r;
    // (a lane without a line walks a line of length 0: it takes part in the cooperative stages and writes nothing -- W = 0 for it)
    apsaraParseLine(src, len, live ? W : 0u, row, r);
    if (live) {
        status[line] = r.status;
        secs[line] = r.secs;
        nanos[line] = r.nanos;
        npairs[line] = r.npairs;
        typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
        i32x4* b = reinterpret_cast<i32x4*>(base + size_t(line) * 8);
        b[0] = i32x4{r.base[0].begin, r.base[0].end, r.base[1].begin, r.base[1].end};
        b[1] = i32x4{r.base[2].begin, r.base[2].end, r.base[3].begin, r.base[3].end};
    }
}

}  // namespace lcapsara
