// csv_kernel.hpp -- csv_split_kernel: the CSV decoder's per-value work on gfx950 (wave64), included by csv_device.hip only.
//
// One value per lane, csvReadRecord() of csv_vm.hpp per lane, through the SOURCE of wave_tile_source.hpp: a wavefront owns a tile of 64
// rows x 64 bytes in LDS (16 KB per 256-thread workgroup), a row is one value's current 64-byte stage, fetched by the whole wavefront
// as aligned 16-byte loads inside the value's own 16-byte units, stage s + 1 in flight while the lanes walk stage s.  The walk is the
// quad-skip form: per 16-byte quad one 16-bit mask each for the separator's first byte, `"`, `\n` and `\r`, a jump to the first set bit
// of the masks the lane's phase cares about.  The separator (1 to 4 bytes) is a constant kernel argument: its further bytes are shifts
// of a scalar register, compared with the value's bytes from the lane's LDS row or, across a stage's border, from memory.
// Results: one status byte, the TRUE field count and the first min(count, W) rows per value, each row ONE 8-byte vector store by the
// value's own lane.  No atomics.
// Two instantiations, TrimLeadingSpace off and on (DESIGN 5.16 has the resource report); neither uses scratch or spills.
#pragma once

#include <hip/hip_runtime.h>

#include "csv_vm.hpp"
#include "wave_tile_source.hpp"

namespace lccsv {

constexpr int kBlock = 256;
static_assert(kCsvStageBytes == lcwave::kWaveStageBytes, "the routine walks the stages WaveTileSource hands out");
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));

// WaveTileSource with the byte reads of csv_vm.hpp: a byte of the value's CURRENT stage comes from the lane's own LDS row (where the
// walk's quads come from), any other one straight from memory (a separator or a white-space rune that straddles the stage's end, the
// `\r` before a `\n` across its start)
struct CsvTileSource : lcwave::WaveTileSource {
    uint32_t current = 0;
    __device__ __forceinline__ CsvTileSource(uint32_t lane_, uint32_t tile_, uintptr_t lineAddr) : lcwave::WaveTileSource(lane_, tile_, lineAddr) {}
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

struct CsvRowSink {
    i32x2* at;  // the value's first row
    uint32_t W;
    __device__ __forceinline__ void field(uint32_t k, int32_t b, int32_t e) {
        if (k < W) at[k] = i32x2{b, e};
    }
};

// (a lane without a value walks a value of length 0 at W = 0: it takes part in the cooperative stages and writes nothing)
template <bool Trim>
__global__ __launch_bounds__(kBlock) void csv_split_kernel(uint32_t sepWord, uint32_t sepLen, const uint8_t* __restrict__ data, const int32_t* __restrict__ off,
                                                           uint32_t n, uint32_t W, uint8_t* __restrict__ status, uint32_t* __restrict__ count,
                                                           int32_t* __restrict__ fields) {
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
    CsvTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    CsvRowSink sink{reinterpret_cast<i32x2*>(fields) + size_t(live ? line : 0u) * W, live ? W : 0u};
    uint8_t st = LC_CSV_OK;
    uint32_t fieldCount = 0;
    csvReadRecord<Trim>(src, sink, len, sepWord, sepLen, &st, &fieldCount);
    if (live) {
        status[line] = st;
        count[line] = fieldCount;
    }
}

}  // namespace lccsv
