// strrep_kernel.hpp -- the gfx950 kernels of the string-replace processor (wave64), included by strrep_device.hip only.  The per-value
// rules are strrep_vm.hpp's, shared with the host; the scan between the two kernels is scan64_kernel.hpp's.
//
//   strrep_size_kernel   one value per lane through the SOURCE of wave_tile_source.hpp, unchanged: a wavefront owns a tile of 64 rows x
//                        64 bytes in LDS (16 KB per 256-thread workgroup), stage s + 1 in flight while the lanes walk stage s.  Per
//                        16-byte unit of its row a lane runs strrepConstUnit / strrepUnquoteUnit with a sink that counts; a needle, an
//                        escape or a UTF-8 sequence that reaches behind the current stage reads those bytes straight from memory
//                        (anchor_kernel.hpp's byteAt), so nothing partial is carried but the cover / the cursor.  Per stage the lane
//                        stores ONE 16-byte vector: its four units' records (bytes produced, skip at entry), and at the end the value's
//                        output length (0 without CHANGED) and flag byte.
//   strrep_write_kernel  kLanes lanes per value (a divisor of 64); a value without LC_STRREP_CHANGED ends at once.  Per round a lane
//                        takes one aligned 16-byte unit of the source and its record; an exclusive prefix over the sub-group places the
//                        lane's bytes, the round's total carries the position on.  The lane then walks its unit from the recorded skip
//                        with a sink that stores (byte stores): no lane waits for another, nothing crosses a unit border but what the
//                        record says, and a long literal run is spread over as many lanes as it has units.
//                        Nothing is stored for an unchanged value, nothing outside [out_off[i], out_off[i + 1]) (the sink is bounded by
//                        the unit's own share), nothing at all when out_off[n] exceeds out_cap.
// Where the records lie: value i's stage s has slot (a_i / 64 + i + s), a_i the value's 16-byte-aligned begin counted from the 64-byte
// boundary at or below d_data; a slot is four words.  Slots of different values never meet: value i + 1 begins at or behind value i's last
// stage begin, and i + 1 > i.  The caller gives room for (extent / 64 + n + 2) slots.
// Plain C++ stores only.  DESIGN.md section 5.21 has the resource report.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "strrep_vm.hpp"
#include "wave_tile_source.hpp"

namespace lcstrrep {

constexpr int kBlock = 256;
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront
constexpr uint32_t kTableWords = sizeof(StrrepConfig) / 4;

typedef const uint8_t __attribute__((address_space(3))) * LdsBytes;

// WaveTileSource with byte reads: a byte of the value's CURRENT stage comes from the lane's own LDS row, any other one straight from memory
struct StrrepTileSource : lcwave::WaveTileSource {
    uint32_t current = 0;
    __device__ __forceinline__ StrrepTileSource(uint32_t lane_, uint32_t tile_, uintptr_t lineAddr) : lcwave::WaveTileSource(lane_, tile_, lineAddr) {}
    __device__ __forceinline__ void stage(uint32_t s) {
        lcwave::WaveTileSource::stage(s);
        current = s;
    }
    __device__ __forceinline__ uint32_t byteAt(uint32_t p) const {
        if (p / lcwave::kWaveStageBytes == current) return *reinterpret_cast<LdsBytes>(myRow + ((p % lcwave::kWaveStageBytes) ^ mySwizzle));
        return lcwave::WaveTileSource::byteAt(p);
    }
};

// the write pass's source: bytes straight from memory (a lane's unit and the few bytes a piece reaches behind it: the same cache lines)
struct StrrepMemorySource {
    uintptr_t rowStart;
    __device__ __forceinline__ uint32_t byteAt(uint32_t p) const { return *reinterpret_cast<const uint8_t*>(rowStart + p); }
};

__device__ __forceinline__ uint64_t recordSlot(uintptr_t data, uintptr_t rowStart, uint32_t i) {
    return uint64_t((rowStart - (data & ~uintptr_t(63))) >> 6) + i;
}

__device__ __forceinline__ void loadTable(const StrrepConfig& cfg, uint32_t* table) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(&cfg);
    for (uint32_t i = threadIdx.x; i < kTableWords; i += kBlock) table[i] = words[i];
    __syncthreads();
}

// sizes: uint64[n + 1] (the scan's input: sizes[n] = 0); records: see above
__global__ __launch_bounds__(kBlock) void strrep_size_kernel(const StrrepConfig cfg, const uint8_t* __restrict__ data, const uint32_t* __restrict__ off,
                                                            uint32_t n, uint8_t* __restrict__ flags, uint64_t* __restrict__ sizes,
                                                            lcwave::u32x4* __restrict__ records) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    __shared__ __attribute__((aligned(16))) uint32_t table[kTableWords];
    loadTable(cfg, table);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t line64 = uint64_t(blockIdx.x) * kBlock + tid;
    const bool live = line64 < n;
    const uint32_t line = live ? uint32_t(line64) : 0u;
    if (line64 == n) sizes[n] = 0;
    uint32_t at = 0, len = 0;
    if (live) {
        at = off[line];
        len = off[line + 1] - at;
    }
    typedef __attribute__((address_space(3))) uint8_t* LdsPtr;
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)tiles)) + wave * kTileBytes;  // LDS byte address
    StrrepTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    const LdsBytes match = (LdsBytes)table;
    const uint32_t head = src.head(), end = head + len;
    const bool isConst = cfg.method == kStrrepConst;
    const uint32_t m = cfg.matchLen, replLen = cfg.replLen;
    // const: the cover and the occurrences so far; unquote: the cursor
    uint32_t cover = head, found = 0;
    StrrepShape shape{};
    bool shaped = true;
    if (!isConst) {
        uint32_t first = 0, last = 0;
        if (len) {
            first = src.lcwave::WaveTileSource::byteAt(head);
            last = src.lcwave::WaveTileSource::byteAt(end - 1);
        }
        shaped = strrepShape(head, len, first, last, &shape);
    }
    StrrepCursor cur{shape.cbegin, 0, shaped ? 0u : 1u, 0};
    uint64_t total = 0;
    lcwave::u32x4* myRecords = records + recordSlot(reinterpret_cast<uintptr_t>(data), src.rowStart, line);
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * lcwave::kWaveStageBytes;
        if (base >= end || !len) continue;  // this lane's value has ended: it only takes part in the cooperative stages
        lcwave::u32x4 rec{0, 0, 0, 0};
#pragma unroll 1
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ub = base + k * 16;
            if (ub >= end) break;
            StrrepCountSink sink;
            sink.replLen = replLen;
            uint32_t skip;
            if (isConst) {
                skip = cover > ub ? cover - ub : 0u;
                uint32_t q[4];
                src.rowQuad(k, q);
                found += strrepConstUnit(match, m, q, ub, end, &cover, src, sink);
            } else {
                skip = cur.p > ub || cur.v ? ((cur.p - ub) << 2) | cur.v : 0u;
                strrepUnquoteUnit(src, shape, ub, &cur, sink);
            }
            const uint32_t r = strrepRecord(sink.bytes, skip);
            rec.x = k == 0 ? r : rec.x;
            rec.y = k == 1 ? r : rec.y;
            rec.z = k == 2 ? r : rec.z;
            rec.w = k == 3 ? r : rec.w;
            total += sink.bytes;
        }
        myRecords[s] = rec;
    }
    if (!live) return;
    uint32_t f = 0;
    if (isConst) f = found ? LC_STRREP_CHANGED : 0u;
    else if (!strrepUnquoteClosed(shape, cur)) f = LC_STRREP_ERROR;
    else if (!shape.formB || cur.escaped) f = LC_STRREP_CHANGED;
    flags[line] = uint8_t(f);
    sizes[line] = (f & LC_STRREP_CHANGED) ? total : 0;
}

template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void strrep_write_kernel(const StrrepConfig cfg, const uint8_t* __restrict__ data, const uint32_t* __restrict__ off,
                                                             uint32_t n, const uint8_t* __restrict__ flags, const uint64_t* __restrict__ outOff,
                                                             const uint32_t* __restrict__ records, uint8_t* __restrict__ out, uint64_t outCap) {
    static_assert(kLanes >= 1 && kLanes <= 64 && (kLanes & (kLanes - 1)) == 0, "lanes per value: a divisor of 64");
    __shared__ __attribute__((aligned(16))) uint32_t table[kTableWords];
    loadTable(cfg, table);
    if (outOff[n] > outCap) return;  // too small: not one byte is stored
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    const uint32_t lane = threadIdx.x % kLanes;
    if (i64 >= n) return;
    const uint32_t i = uint32_t(i64);
    if (!(flags[i] & LC_STRREP_CHANGED)) return;  // (the same in every lane of the sub-group)
    const uint32_t at = off[i], len = off[i + 1] - at;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(data) + at;
    const uint32_t head = uint32_t(addr & 15u), end = head + len;
    const StrrepMemorySource src{addr - head};
    const uint32_t units = (end + 15) / 16;
    const uint32_t* myRecords = records + recordSlot(reinterpret_cast<uintptr_t>(data), src.rowStart, i) * 4;
    const bool isConst = cfg.method == kStrrepConst;
    StrrepShape shape{};
    if (!isConst) strrepShape(head, len, len ? src.byteAt(head) : 0u, len ? src.byteAt(end - 1) : 0u, &shape);
    uint64_t pos = outOff[i];
    const uint64_t limit = outOff[i + 1];
    for (uint32_t first = 0; first < units; first += kLanes) {  // a round of the sub-group (the same trip count in all of its lanes)
        const uint32_t u = first + lane;
        const uint32_t rec = u < units ? myRecords[u] : 0u;
        const uint32_t own = strrepRecordBytes(rec);
        uint32_t incl = own;
#pragma unroll
        for (uint32_t d = 1; d < kLanes; d <<= 1) {
            const uint32_t up = uint32_t(__shfl_up(int(incl), d, int(kLanes)));
            if (lane >= d) incl += up;
        }
        if (own) {
            const uint64_t mine = pos + (incl - own);
            const uint64_t stop = mine + own < limit ? mine + own : limit;
            StrrepStoreSink<LdsBytes> sink{out + mine, out + stop, (LdsBytes)table + kStrrepReplAt, cfg.replLen};
            const uint32_t ub = u * 16, skip = strrepRecordSkip(rec);
            if (isConst) {
                const lcwave::u32x4 v = *reinterpret_cast<lcwave::GlobalQuadPtr>(src.rowStart + ub);
                const uint32_t q[4] = {v.x, v.y, v.z, v.w};
                uint32_t cover = ub + skip;
                strrepConstUnit((LdsBytes)table, cfg.matchLen, q, ub, end, &cover, src, sink);
            } else {
                StrrepCursor cur{ub + (skip >> 2), skip & 3u, 0, 0};
                strrepUnquoteUnit(src, shape, ub, &cur, sink);
            }
        }
        pos += uint32_t(__shfl(int(incl), int(kLanes - 1), int(kLanes)));
    }
}

}  // namespace lcstrrep
