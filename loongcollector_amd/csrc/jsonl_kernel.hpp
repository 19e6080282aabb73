// jsonl_kernel.hpp -- the gfx950 kernels of the JSON-lines encoder (launched by jsonl_device.hip; the per-event rules and the unit
// functions are jsonl_vm.hpp's, shared with the host; the scan is scan64_kernel.hpp's):
//   jsonl_size_kernel    kLanes lanes per event.  Per item the lanes take the value's aligned 16-byte units in turn and classify them;
//                        the sub-group reduces to the first NUL (a minimum) and the two-byte and six-byte counts in front of it -> the
//                        record's size (0: no record) and, per item, (raw length, escaped length) for the write pass
//   jsonl_write_kernel   kLanes lanes per event, piece by piece at a running position that is the same in every lane:
//                          copied pieces (head, item prefixes, CLEAN values: escaped length == raw length) -- a lane owns aligned dwords
//                            of the output, one 4-byte store per word inside the piece, consecutive lanes store consecutive words
//                          DIRTY values -- source-owned: per round a lane takes a unit, an exclusive prefix over the sub-group places it,
//                            the lane emits its bytes (byte stores); the round's total carries the position on
//                          the time's digits, the closing quote and `}\n` -- single byte stores
//                        Nothing is stored when the total exceeds out_cap.
// A sub-group's loops (items, rounds) have the same trip count in all of its lanes, so every shuffle finds its sub-group whole.
// Plain C++ stores only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "jsonl_vm.hpp"

namespace lcjsonl {

constexpr uint32_t kBlock = 256;

// what lc_regex_match_device left behind, the events' times and the group's head
struct JsonlBatch {
    const uint8_t* data;
    const uint32_t* off;
    const uint32_t* len;  // may be null: len[i] = off[i + 1] - off[i] - sep
    uint32_t sep, n, ngroups;
    const int32_t* caps;
    const uint8_t* status;
    const uint32_t* time;
    const uint8_t* head;  // 4-byte aligned
    uint32_t headLen;
    uint32_t itemStride;  // rows of itemLens per event: the longer list's items
};

__device__ __forceinline__ JsonlEvent loadEvent(const JsonlPlanView& P, const JsonlBatch& b, uint32_t i) {
    JsonlEvent e;
    const uint32_t at = b.off[i];
    if (b.len) {
        e.lineLen = b.len[i];
    } else {
        const uint32_t span = b.off[i + 1] - at;
        e.lineLen = span >= b.sep ? span - b.sep : 0;
    }
    e.line = b.data + at;
    e.caps = b.caps + size_t(i) * 2 * b.ngroups;
    eventItems(P, b.status[i], &e.firstItem, &e.nItems);
    e.time = b.time[i];
    return e;
}

// the aligned 16-byte units that overlap v[0 .. len), len > 0: unit u covers value bytes [16 u - skew, 16 u - skew + 16)
struct ValueUnits {
    const uint4* base;
    uint32_t skew;
    uint32_t count;
};
__device__ __forceinline__ ValueUnits unitsOf(const uint8_t* v, uint32_t len) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(v);
    ValueUnits u;
    u.skew = uint32_t(a & 15u);
    u.base = reinterpret_cast<const uint4*>(a - u.skew);
    u.count = uint32_t((uint64_t(u.skew) + len + 15) >> 4);
    return u;
}
// unit k of the value, classified: which of its bytes are the value's
__device__ __forceinline__ UnitMasks loadUnit(const ValueUnits& u, uint32_t len, uint32_t k, uint32_t w[4]) {
    const uint4 x = u.base[k];
    w[0] = x.x;
    w[1] = x.y;
    w[2] = x.z;
    w[3] = x.w;
    const uint64_t first = uint64_t(k) * 16;  // (in skewed positions: the value is [skew, skew + len))
    const uint32_t lo = first < u.skew ? u.skew - uint32_t(first) : 0;
    const uint64_t endAt = uint64_t(u.skew) + len;
    const uint32_t hi = endAt - first < 16 ? uint32_t(endAt - first) : 16;
    return classifyUnit(w, lo, hi);
}

template <uint32_t kLanes>
__device__ __forceinline__ uint32_t groupMin(uint32_t v) {
#pragma unroll
    for (uint32_t d = kLanes / 2; d >= 1; d >>= 1) {
        const uint32_t o = uint32_t(__shfl_xor(int(v), int(d), int(kLanes)));
        v = o < v ? o : v;
    }
    return v;
}
template <uint32_t kLanes>
__device__ __forceinline__ uint32_t groupSum(uint32_t v) {
#pragma unroll
    for (uint32_t d = kLanes / 2; d >= 1; d >>= 1) v += uint32_t(__shfl_xor(int(v), int(d), int(kLanes)));
    return v;
}

// one lane's part of v[0 .. len): its units' two-byte and six-byte counts up to ITS first NUL, and where that NUL stands (len: none)
template <uint32_t kLanes>
__device__ __forceinline__ void countLane(const uint8_t* v, uint32_t len, uint32_t lane, uint32_t* two, uint32_t* six, uint32_t* nulAt) {
    uint32_t c2 = 0, c6 = 0, nul = len;
    if (len) {
        const ValueUnits u = unitsOf(v, len);
        for (uint32_t k = lane; k < u.count; k += kLanes) {
            uint32_t w[4];
            const UnitMasks m = loadUnit(u, len, k, w);
            const uint32_t live = liveBytes(m);
            c2 += popc32(m.two & live);
            c6 += popc32(m.six & live);
            if (m.nul) {
                nul = k * 16 + ctz32(m.nul) - u.skew;
                break;
            }
        }
    }
    *two = c2;
    *six = c6;
    *nulAt = nul;
}

// the whole sub-group's answer for v[0 .. len): the length in front of the first NUL and the escaped length of that
template <uint32_t kLanes>
__device__ __forceinline__ void scanValueLanes(const uint8_t* v, uint32_t len, uint32_t lane, uint32_t* rawLen, uint64_t* escLen) {
    uint32_t c2, c6, nul;
    countLane<kLanes>(v, len, lane, &c2, &c6, &nul);
    const uint32_t raw = groupMin<kLanes>(nul);
    if (raw < len) countLane<kLanes>(v, raw, lane, &c2, &c6, &nul);  // bytes behind the first NUL were counted by other lanes: once more, cut
    *rawLen = raw;
    *escLen = uint64_t(raw) + groupSum<kLanes>(c2) + 5ull * groupSum<kLanes>(c6);
}

// itemLens: uint32[n][itemStride][2] = (raw length, escaped length) per item, or null
template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void jsonl_size_kernel(JsonlPlanView P, JsonlBatch b, uint64_t* __restrict__ sizes, uint32_t* __restrict__ itemLens) {
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    const uint32_t lane = threadIdx.x % kLanes;
    if (i64 > b.n) return;
    if (i64 == b.n) {  // the scan's last element: rec_off[n] becomes the total
        if (lane == 0) sizes[i64] = 0;
        return;
    }
    const uint32_t i = uint32_t(i64);
    const JsonlEvent e = loadEvent(P, b, i);
    uint64_t size = e.nItems ? uint64_t(b.headLen) + decimalDigits(e.time) + 2 : 0;
    for (uint32_t k = 0; k < e.nItems; ++k) {
        const JsonlItem it = P.items[e.firstItem + k];
        uint32_t vb, len, raw;
        uint64_t esc;
        itemValue(e, it.source, &vb, &len);
        scanValueLanes<kLanes>(e.line + vb, len, lane, &raw, &esc);
        size += uint64_t(it.prefixLen) + esc + 1;
        if (itemLens && lane == 0) {
            uint32_t* row = itemLens + (size_t(i) * b.itemStride + k) * 2;
            row[0] = raw;
            row[1] = uint32_t(esc < 0xFFFFFFFFull ? esc : 0xFFFFFFFFull);  // (beyond: the record is not written)
        }
    }
    if (lane == 0) sizes[i] = size >= kMaxRecordBytes ? 0 : size;
}

// a dirty value, source-owned: v[0 .. rawLen) (no NUL in it) escaped to out[pos ..); returns the position behind it
template <uint32_t kLanes>
__device__ __forceinline__ uint64_t emitDirtyLanes(uint8_t* out, uint64_t pos, const uint8_t* v, uint32_t rawLen, uint32_t lane) {
    const ValueUnits u = unitsOf(v, rawLen);
    for (uint32_t first = 0; first < u.count; first += kLanes) {  // a round of the sub-group
        const uint32_t k = first + lane;
        uint32_t w[4] = {0, 0, 0, 0};
        UnitMasks m{0, 0, 0, 0};
        if (k < u.count) m = loadUnit(u, rawLen, k, w);
        const uint32_t own = escapedBytes(m, m.valid);
        uint32_t incl = own;
#pragma unroll
        for (uint32_t d = 1; d < kLanes; d <<= 1) {
            const uint32_t up = uint32_t(__shfl_up(int(incl), d, int(kLanes)));
            if (lane >= d) incl += up;
        }
        if (own) emitUnit(out + pos + (incl - own), w, m, m.valid);
        pos += uint32_t(__shfl(int(incl), int(kLanes - 1), int(kLanes)));
    }
    return pos;
}

// kLanes lanes per event (a divisor of 64); out is 16-byte aligned.  itemLens: what the size kernel stored, or null (derived again here)
template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void jsonl_write_kernel(JsonlPlanView P, JsonlBatch b, const uint64_t* __restrict__ recOff,
                                                             const uint32_t* __restrict__ itemLens, uint8_t* __restrict__ out, uint64_t outCap,
                                                             uint64_t* __restrict__ totalOut) {
    // (the host entry's trip: the total goes where the host reads it, through the pinned mapping)
    if (totalOut && blockIdx.x == 0 && threadIdx.x == 0) *totalOut = recOff[b.n];
    if (recOff[b.n] > outCap) return;  // too small: not one byte is stored
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    const uint32_t lane = threadIdx.x % kLanes;
    if (i64 >= b.n) return;
    const uint32_t i = uint32_t(i64);
    uint64_t pos = recOff[i];
    if (recOff[i + 1] == pos) return;
    const JsonlEvent e = loadEvent(P, b, i);
    copyPieceLanes(out, pos, b.headLen, b.head, lane, kLanes);
    pos += b.headLen;
    const uint32_t nd = decimalDigits(e.time);
    for (uint32_t j = lane; j < nd; j += kLanes) out[pos + j] = decimalDigit(e.time, nd, j);
    pos += nd;
    for (uint32_t k = 0; k < e.nItems; ++k) {
        const JsonlItem it = P.items[e.firstItem + k];
        copyPieceLanes(out, pos, it.prefixLen, P.blob + it.prefixAt, lane, kLanes);
        pos += it.prefixLen;
        uint32_t vb, len, raw;
        uint64_t esc;
        itemValue(e, it.source, &vb, &len);
        if (itemLens) {
            const uint32_t* row = itemLens + (size_t(i) * b.itemStride + k) * 2;
            raw = row[0];
            esc = row[1];
        } else {
            scanValueLanes<kLanes>(e.line + vb, len, lane, &raw, &esc);
        }
        if (esc == raw) {
            copyPieceLanes(out, pos, raw, e.line + vb, lane, kLanes);
            pos += raw;
        } else {
            pos = emitDirtyLanes<kLanes>(out, pos, e.line + vb, raw, lane);
        }
        if (lane == kLanes - 1) out[pos] = '"';
        ++pos;
    }
    if (lane == 0) out[pos] = '}';
    if (lane == 1 % kLanes) out[pos + 1] = '\n';
}

}  // namespace lcjsonl
