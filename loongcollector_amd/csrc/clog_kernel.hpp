// clog_kernel.hpp -- clog_containerd_kernel and clog_docker_kernel: the container stdout parser's per-line work on gfx950 (wave64),
// included by clog_device.hip only.
//
// One line per lane, the routines of clog_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of 64 rows
// x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one line's current 64-byte stage, fetched by the whole wavefront as
// aligned 16-byte loads inside the line's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.
//   clog_docker_kernel       walks whole lines; the unescaped text of a "log" value goes to the shadow buffer as byte stores of the
//                            line's own lane, at the value's own offset.  The last byte of a line (the reference's first test) is
//                            the one byte read out of order, straight from memory.
//   clog_containerd_kernel   stages only while some lane of the wavefront has not seen the byte two behind its second blank: normally
//                            ONE stage, whatever the contents' length (the prefetch of the stage behind it is the only other traffic).
// Results: per line one status byte, one flag byte, three (begin, end) spans as three 8-byte stores, rewrite_begin; all by the line's
// own lane as plain vector stores.  No atomics.
#pragma once

#include <hip/hip_runtime.h>

#include "clog_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcclog {

constexpr int kBlock = 256;
static_assert(kClogStageBytes == lcwave::kWaveStageBytes, "the routines walk the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront

struct ClogTileSource : lcwave::WaveTileSource {
    using lcwave::WaveTileSource::WaveTileSource;
    __device__ __forceinline__ bool anyLane(bool mine) const { return __any(mine) != 0; }
};

struct ClogShadowSink {
    uint8_t* at;  // the line's first byte in the shadow buffer
    __device__ __forceinline__ void put(uint32_t pos, uint32_t byte) { at[pos] = uint8_t(byte); }
};

__device__ __forceinline__ void clogStore(const ClogLine& r, uint32_t line, uint8_t* __restrict__ status, uint8_t* __restrict__ flags,
                                          int32_t* __restrict__ spans, int32_t* __restrict__ rewriteBegin) {
    status[line] = r.status;
    flags[line] = r.flags;
    rewriteBegin[line] = r.rewriteBegin;
    typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
    i32x2* s = reinterpret_cast<i32x2*>(spans + size_t(line) * 6);
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = i32x2{r.span[k].begin, r.span[k].end};
}

#define LC_CLOG_KERNEL_PROLOGUE                                                                                             \
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];                                      \
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;                                                    \
    const uint32_t line = blockIdx.x * kBlock + tid;                                                                        \
    const bool live = line < n;                                                                                             \
    uint32_t o = 0, len = 0;                                                                                                \
    if (live) {                                                                                                             \
        o = uint32_t(off[line]);                                                                                            \
        len = uint32_t(off[line + 1]) - o;                                                                                  \
    }                                                                                                                       \
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;                                                              \
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * kTileBytes; /* LDS byte address */ \
    ClogTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + o);                                                  \
    ClogLine r;

// (a lane without a line walks a line of length 0: it takes part in the cooperative stages and writes nothing)
__global__ __launch_bounds__(kBlock) void clog_containerd_kernel(const uint8_t* __restrict__ data, const int32_t* __restrict__ off, uint32_t n,
                                                                 uint8_t* __restrict__ status, uint8_t* __restrict__ flags,
                                                                 int32_t* __restrict__ spans, int32_t* __restrict__ rewriteBegin) {
    LC_CLOG_KERNEL_PROLOGUE
    clogParseContainerd(src, len, r);
    if (live) clogStore(r, line, status, flags, spans, rewriteBegin);
}

__global__ __launch_bounds__(kBlock) void clog_docker_kernel(const uint8_t* __restrict__ data, const int32_t* __restrict__ off, uint32_t n,
                                                             uint8_t* __restrict__ status, uint8_t* __restrict__ flags,
                                                             int32_t* __restrict__ spans, int32_t* __restrict__ rewriteBegin,
                                                             uint8_t* __restrict__ shadow) {
    LC_CLOG_KERNEL_PROLOGUE
    ClogShadowSink sink{shadow + o};
    clogParseDocker(src, sink, len, r);
    if (live) clogStore(r, line, status, flags, spans, rewriteBegin);
}

#undef LC_CLOG_KERNEL_PROLOGUE

}  // namespace lcclog
