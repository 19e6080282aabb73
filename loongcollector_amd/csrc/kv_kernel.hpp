// kv_kernel.hpp -- kv_split_kernel: the key-value splitter's per-value work on gfx950 (wave64), included by kv_device.hip only.
//
// One value per lane, kvSplitLine() of kv_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of 64
// rows x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one value's current 64-byte stage, fetched by the whole wavefront
// as aligned 16-byte loads inside the value's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.  The walk is the
// quad-skip form: per 16-byte quad one 16-bit mask per needle, a jump to the first set bit of the masks the lane's phase cares about,
// longer needles confirmed only there (kv_vm.hpp), from the lane's LDS row or, across a stage's border, from memory (KvTileSource).
// The needles (up to 32 bytes each) arrive as constant kernel arguments and are copied to 96 bytes of LDS once per workgroup: a lane
// reads a needle's further bytes from there, never from registers of its own.
// Results: one status byte, the TRUE pair count and the first min(count, W) rows per value, each row ONE 16-byte vector store by the
// value's own lane.  No atomics.
// Three instantiations (DESIGN 5.15 has the resource report and what the third buys): kKvQuoteNone has no extension logic and no second
// walk (66 VGPRs, 7 waves per SIMD); kKvQuoteOne keeps notes of the quotes it passed (94 VGPRs, 5 waves); kKvQuoteLong compares the
// quote's bytes (92 VGPRs, 5 waves).  None uses scratch or spills.
#pragma once

#include <hip/hip_runtime.h>

#include "kv_vm.hpp"
#include "wave_tile_source.hpp"

namespace lckv {

constexpr int kBlock = 256;
static_assert(kKvStageBytes == lcwave::kWaveStageBytes, "the routine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront
constexpr uint32_t kNeedleBytes = 3 * LC_KV_MAX_NEEDLE;
static_assert(offsetof(KvConfig, delim) == 0 && offsetof(KvConfig, sep) == LC_KV_MAX_NEEDLE && offsetof(KvConfig, quote) == 2 * LC_KV_MAX_NEEDLE &&
                  kNeedleBytes % 4 == 0,
              "the needles are the first 96 bytes of the config");

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// the config's needle bytes as words: a kernel argument of its own, so that a thread picks ITS word with a select chain over scalar
// registers and nothing is indexed in memory
struct KvNeedleWords {
    uint32_t w[kNeedleBytes / 4];
};

// WaveTileSource with the byte reads of kv_vm.hpp: a byte of the value's CURRENT stage comes from the lane's own LDS row (where the
// walk's quads come from), any other one straight from memory (a needle that straddles the stage's end, a look-back across its start)
struct KvTileSource : lcwave::WaveTileSource {
    uint32_t current = 0;
    __device__ __forceinline__ KvTileSource(uint32_t lane_, uint32_t tile_, uintptr_t lineAddr) : lcwave::WaveTileSource(lane_, tile_, lineAddr) {}
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

struct KvRowSink {
    i32x4* at;  // the value's first row
    uint32_t W;
    __device__ __forceinline__ void pair(uint32_t k, int32_t kb, int32_t ke, int32_t vb, int32_t ve) {
        if (k < W) at[k] = i32x4{kb, ke, vb, ve};
    }
};

// (a lane without a value walks a value of length 0 at W = 0: it takes part in the cooperative stages and writes nothing)
template <int QM>
__global__ __launch_bounds__(kBlock) void kv_split_kernel(KvNeedleWords words, uint32_t delimLen, uint32_t sepLen, uint32_t quoteLen,
                                                          const uint8_t* __restrict__ data, const int32_t* __restrict__ off, uint32_t n, uint32_t W,
                                                          uint8_t* __restrict__ status, uint32_t* __restrict__ npairs, int32_t* __restrict__ pairs) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    __shared__ __attribute__((aligned(16))) uint32_t needles[kNeedleBytes / 4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < kNeedleBytes / 4) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t i = 0; i < kNeedleBytes / 4; ++i) mine = tid == i ? words.w[i] : mine;
        needles[tid] = mine;
    }
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
    KvTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    const KvNeedles nd = kvNeedles(reinterpret_cast<const uint8_t*>(needles), delimLen, sepLen, quoteLen, words.w[0] & 0xFFu,
                                   words.w[LC_KV_MAX_NEEDLE / 4] & 0xFFu, words.w[2 * LC_KV_MAX_NEEDLE / 4] & 0xFFu);
    KvRowSink sink{reinterpret_cast<i32x4*>(pairs) + size_t(live ? line : 0u) * W, live ? W : 0u};
    uint8_t st = LC_KV_OK;
    uint32_t count = 0;
    kvSplitLine<QM>(nd, src, sink, len, &st, &count);
    if (live) {
        status[line] = st;
        npairs[line] = count;
    }
}

}  // namespace lckv
