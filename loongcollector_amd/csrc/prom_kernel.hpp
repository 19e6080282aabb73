// prom_kernel.hpp -- prom_parse_kernel: the Prometheus text-line parser's per-line work on gfx950 (wave64), included by prom_device.hip
// only.
//
// One line per lane, promParseLine() of prom_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of 64
// rows x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one line's current 64-byte stage, fetched by the whole wavefront as
// aligned 16-byte loads inside the line's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.
// Results: structure of arrays, every entry written by the line's own lane as plain vector stores (spans as 8-byte vectors, a label as
// ONE 16-byte vector, and only labels below W).  No atomics.  A number is converted by the lane where one rounded operation gives
// strtod's answer; every other token leaves as a flag and a span.
#pragma once

#include <hip/hip_runtime.h>

#include "prom_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcprom {

constexpr int kBlock = 256;
static_assert(kPromStageBytes == lcwave::kWaveStageBytes, "the routine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

struct PromLabelSink {
    i32x4* at;  // the line's first label entry
    uint32_t W;
    __device__ __forceinline__ void label(uint32_t k, int32_t nb, int32_t ne, int32_t vb, int32_t ve) {
        if (k < W) at[k] = i32x4{nb, ne, vb, ve};
    }
};

struct PromOut {
    uint8_t* status;
    uint8_t* flags;
    int32_t* name;
    uint64_t* value;
    int32_t* valueSpan;
    int32_t* timeSpan;
    int64_t* secs;
    uint32_t* nanos;
    uint32_t* nlabels;
    int32_t* labels;
};

// (a lane without a line walks a line of length 0: it takes part in the cooperative stages and writes nothing)
// Three waves per SIMD: the machine is one long chain of divergent branches, and the compiler's own choice (169 VGPRs) misses the third
// wave by one register; held to 168 it spills nothing.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3, 3))) void prom_parse_kernel(const uint8_t* __restrict__ data,
                                                                                                       const int32_t* __restrict__ off, uint32_t n,
                                                                                                       uint32_t W, int honor, PromOut o) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t line = blockIdx.x * kBlock + tid;
    const bool live = line < n;
    uint32_t at = 0, len = 0;
    if (live) {
        at = uint32_t(off[line]);
        len = uint32_t(off[line + 1]) - at;
    }
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * kTileBytes;  // LDS byte address
    lcwave::WaveTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    // (a lane without a line never reaches label(): its line is empty)
    PromLabelSink sink{reinterpret_cast<i32x4*>(o.labels) + size_t(live ? line : 0u) * W, live ? W : 0u};
    PromLine r;
    promParseLine(src, sink, len, honor != 0, r);
    if (!live) return;
    o.status[line] = r.status;
    o.flags[line] = r.flags;
    reinterpret_cast<i32x2*>(o.name)[line] = i32x2{r.name.begin, r.name.end};
    o.value[line] = r.value;
    reinterpret_cast<i32x2*>(o.valueSpan)[line] = i32x2{r.valueSpan.begin, r.valueSpan.end};
    reinterpret_cast<i32x2*>(o.timeSpan)[line] = i32x2{r.timeSpan.begin, r.timeSpan.end};
    o.secs[line] = r.secs;
    o.nanos[line] = r.nanos;
    o.nlabels[line] = r.nlabels;
}

}  // namespace lcprom
