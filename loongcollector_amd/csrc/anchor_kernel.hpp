// anchor_kernel.hpp -- anchor_locate_kernel: the anchor processor's per-value work on gfx950 (wave64), included by anchor_device.hip only.
//
// One value per lane, anchorLocate() of anchor_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of
// 64 rows x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one value's current 64-byte stage, fetched by the whole
// wavefront as aligned 16-byte loads inside the value's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.  The
// walk is the quad-skip form for up to 16 needle pairs at once (anchor_vm.hpp); a wavefront whose lanes have all resolved all their
// anchors leaves the stage loop, so the rest of its values is never fetched.
// The configuration (needles, one word of first bytes and lengths per anchor, count: 1092 bytes) arrives as constant kernel arguments;
// needles and words are copied to LDS once per workgroup: every lane reads an anchor's word from the same LDS address (so it is
// wave-uniform without holding 16 of them in scalar registers), a needle's further bytes from there too, all as LDS reads.
// Results: the value's row of S (begin, end) entries, written by the value's own lane: a begin and an end the moment the walk knows
// them, (code, -1) for what is still open at the value's end and for the pad entry.  No atomics.  DESIGN 5.18 has the resource report.
#pragma once

#include <hip/hip_runtime.h>

#include "anchor_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcanchor {

constexpr int kBlock = 256;
static_assert(kAnchorStageBytes == lcwave::kWaveStageBytes, "the routine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront
static_assert(offsetof(AnchorConfig, start) == 0 && offsetof(AnchorConfig, stop) == kAnchorNeedleBytes / 2 &&
                  offsetof(AnchorConfig, meta) == kAnchorNeedleBytes && offsetof(AnchorConfig, count) == kAnchorTableBytes &&
                  kAnchorTableBytes % 4 == 0,
              "the needle table is the first 1088 bytes of the config");

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));

// WaveTileSource with the byte reads of anchor_vm.hpp: a byte of the value's CURRENT stage comes from the lane's own LDS row (where
// the walk's quads come from), any other one straight from memory (a needle that straddles the stage's end)
struct AnchorTileSource : lcwave::WaveTileSource {
    uint32_t current = 0;
    __device__ __forceinline__ AnchorTileSource(uint32_t lane_, uint32_t tile_, uintptr_t lineAddr) : lcwave::WaveTileSource(lane_, tile_, lineAddr) {}
    __device__ __forceinline__ void stage(uint32_t s) {
        lcwave::WaveTileSource::stage(s);
        current = s;
    }
    __device__ __forceinline__ uint32_t byteAt(uint32_t p) const {
        typedef const uint8_t __attribute__((address_space(3))) * LdsBytePtr;
        if (p / lcwave::kWaveStageBytes == current) return *reinterpret_cast<LdsBytePtr>(myRow + ((p % lcwave::kWaveStageBytes) ^ mySwizzle));
        return lcwave::WaveTileSource::byteAt(p);
    }
};

struct AnchorRowSink {
    int32_t* row;  // the value's row
    bool live;
    __device__ __forceinline__ void begin(uint32_t a, int32_t b) {
        if (live) row[2 * a] = b;
    }
    __device__ __forceinline__ void end(uint32_t a, int32_t e) {
        if (live) row[2 * a + 1] = e;
    }
    __device__ __forceinline__ void none(uint32_t a, int32_t code) {
        if (live) reinterpret_cast<i32x2*>(row)[a] = i32x2{code, -1};
    }
};

// (a lane without a value walks a value of length 0 with a sink that drops everything: it takes part in the cooperative stages)
__global__ __launch_bounds__(kBlock) void anchor_locate_kernel(const AnchorConfig cfg, const uint8_t* __restrict__ data, const int32_t* __restrict__ off,
                                                               uint32_t n, uint32_t S, int32_t* __restrict__ spans) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    __shared__ __attribute__((aligned(16))) uint32_t table[kAnchorTableBytes / 4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(&cfg);
    for (uint32_t i = tid; i < kAnchorTableBytes / 4; i += kBlock) table[i] = words[i];
    __syncthreads();
    const uint32_t line = blockIdx.x * kBlock + tid;
    const bool live = line < n;
    uint32_t at = 0, len = 0;
    if (live) {
        at = uint32_t(off[line]);
        len = uint32_t(off[line + 1]) - at;
    }
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * kTileBytes;  // LDS byte address
    AnchorTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    AnchorRowSink sink{spans + size_t(live ? line : 0u) * S * 2, live};
    typedef const uint8_t __attribute__((address_space(3))) * LdsBytes;
    typedef const uint32_t __attribute__((address_space(3))) * LdsWords;
    anchorLocate((LdsBytes)table, (LdsWords)table + kAnchorNeedleBytes / 4, cfg.count, src, sink, len);
}

}  // namespace lcanchor
