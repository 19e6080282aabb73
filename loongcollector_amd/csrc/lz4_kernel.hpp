// lz4_kernel.hpp -- the gfx950 kernels of the LZ4 block writer (launched by lz4_device.hip; the rules are lz4_vm.hpp's, shared with the
// host).  The segment lengths live on the device, so no launch is sized by them: every kernel walks its work with a grid stride and reads
// the counts from the head the first kernel leaves in the scratch.
//   lz4_plan_kernel    one workgroup: chunks and match slots per segment, their exclusive scans, the scratch layout -> Lz4Head; refuses
//                      (ok = 0, every d_out_off entry = ~0) a segment at or above the limit and a scratch that is too small
//   lz4_match_kernel   one wavefront per chunk, a hash table of its own in LDS: the steps of lz4_vm.hpp -> the chunk's matches, their
//                      count, the end of its last match
//   lz4_scan_*         64-bit exclusive scan over the chunks, a maximum (the end of the last match in front of a chunk) or a sum (where a
//                      chunk's bytes begin): tile sums, one workgroup over the sums, tile scan -- sls_kernel.hpp's three launches, restated
//   lz4_size_kernel    one wavefront per chunk: the bytes its sequences take, the segment's closing sequence with its last chunk
//   lz4_emit_kernel    one wavefront per chunk, kLanes lanes per sequence; a lane owns ALIGNED dwords of the output and assembles each
//                      (lz4SeqWord): a word inside a sequence is one 4-byte store, a word inside the literals one load and one store; only a
//                      sequence's first and last partial word are byte stores.  Nothing is stored when the total exceeds out_cap.
// Plain C++ stores and LDS atomics only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lz4_vm.hpp"

namespace lclz4 {

constexpr uint32_t kMatchBlock = 128;  // 2 wavefronts, 32 KiB of LDS: five workgroups per CU
constexpr uint32_t kBlock = 256;
constexpr uint32_t kScanPerThread = 4;
constexpr uint32_t kScanTile = kBlock * kScanPerThread;
constexpr uint32_t kScanTilesPerPass = 1024;
constexpr uint32_t kPlanBlock = 1024;

// where the arrays lie in the scratch, for nSeg segments that make `chunks` chunks and `slots` match slots
struct Lz4Layout {
    uint64_t chunkBaseAt, slotBaseAt;  // uint64[nSeg + 1] each: a function of nSeg alone
    uint64_t cntAt;                    // uint32[chunks]
    uint64_t maxAt, sizeAt;            // uint64[chunks + 1] each
    uint64_t tileAt;                   // uint64[tiles]
    uint64_t matchAt;                  // Lz4Match[slots]
    uint64_t bytes;
};
struct Lz4Head {
    uint64_t chunks, slots;
    uint32_t ok, pad;
    Lz4Layout L;
};
LC_LZ4_HD uint64_t lz4Up(uint64_t v) { return (v + 255) / 256 * 256; }
LC_LZ4_HD uint64_t lz4Tiles(uint64_t chunks) { return (chunks + 1 + kScanTile - 1) / kScanTile; }
LC_LZ4_HD Lz4Layout lz4Layout(uint64_t nSeg, uint64_t chunks, uint64_t slots) {
    Lz4Layout L;
    L.chunkBaseAt = 256;
    L.slotBaseAt = L.chunkBaseAt + lz4Up((nSeg + 1) * 8);
    L.cntAt = L.slotBaseAt + lz4Up((nSeg + 1) * 8);
    L.maxAt = L.cntAt + lz4Up(chunks * 4);
    L.sizeAt = L.maxAt + lz4Up((chunks + 1) * 8);
    L.tileAt = L.sizeAt + lz4Up((chunks + 1) * 8);
    L.matchAt = L.tileAt + lz4Up(lz4Tiles(chunks) * 8);
    L.bytes = L.matchAt + lz4Up(slots * 8);
    return L;
}
// a segment's chunks (an empty segment has one, which holds its closing byte) and match slots (a chunk of L bytes finds at most L / 4)
LC_LZ4_HD uint64_t lz4SegChunks(uint32_t len, uint32_t C) { return len ? (uint64_t(len) + C - 1) / C : 1; }
LC_LZ4_HD uint64_t lz4SegSlots(uint32_t len) { return len / 4 + 1; }

struct Lz4Job {
    const uint8_t* in;
    const uint64_t* segBegin;
    const uint32_t* segLen;
    uint32_t nSeg, C;
    uint8_t* scratch;
};

__device__ __forceinline__ uint64_t waveInclusive(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= uint32_t(d)) v += up;
    }
    return v;
}

__global__ __launch_bounds__(kPlanBlock) void lz4_plan_kernel(Lz4Job j, uint64_t scratchBytes, uint64_t* __restrict__ outOff) {
    __shared__ uint64_t waveA[kPlanBlock / 64], waveB[kPlanBlock / 64];
    __shared__ uint64_t carryA, carryB;
    __shared__ uint32_t bad;
    const Lz4Layout L0 = lz4Layout(j.nSeg, 0, 0);  // (the host has checked that the scratch holds this much)
    uint64_t* chunkBase = reinterpret_cast<uint64_t*>(j.scratch + L0.chunkBaseAt);
    uint64_t* slotBase = reinterpret_cast<uint64_t*>(j.scratch + L0.slotBaseAt);
    if (threadIdx.x == 0) carryA = carryB = 0, bad = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < j.nSeg; base += kPlanBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t len = i < j.nSeg ? j.segLen[i] : 0;
        if (len >= kLz4SegLimit) atomicOr(&bad, 1u);
        const uint64_t a = i < j.nSeg ? lz4SegChunks(len, j.C) : 0, b = i < j.nSeg ? lz4SegSlots(len) : 0;
        const uint64_t inclA = waveInclusive(a, lane), inclB = waveInclusive(b, lane);
        if (lane == 63) waveA[wave] = inclA, waveB[wave] = inclB;
        __syncthreads();
        uint64_t beforeA = carryA, beforeB = carryB;
        for (uint32_t w = 0; w < wave; ++w) beforeA += waveA[w], beforeB += waveB[w];
        if (i < j.nSeg) chunkBase[i] = beforeA + inclA - a, slotBase[i] = beforeB + inclB - b;
        __syncthreads();
        if (threadIdx.x == kPlanBlock - 1) carryA = beforeA + inclA, carryB = beforeB + inclB;
        __syncthreads();
    }
    __shared__ uint32_t ok;
    if (threadIdx.x == 0) {
        Lz4Head* H = reinterpret_cast<Lz4Head*>(j.scratch);
        chunkBase[j.nSeg] = carryA;
        slotBase[j.nSeg] = carryB;
        H->chunks = carryA;
        H->slots = carryB;
        H->L = lz4Layout(j.nSeg, carryA, carryB);
        H->ok = ok = (!bad && H->L.bytes <= scratchBytes) ? 1u : 0u;
        H->pad = 0;
    }
    __syncthreads();
    if (!ok)
        for (uint32_t i = threadIdx.x; i <= j.nSeg; i += kPlanBlock) outOff[i] = ~uint64_t(0);
}

// the segment of chunk c: the last s with chunkBase[s] <= c
__device__ __forceinline__ uint32_t segmentOf(const uint64_t* __restrict__ chunkBase, uint32_t nSeg, uint64_t c) {
    uint32_t lo = 0, hi = nSeg;  // chunkBase[lo] <= c < chunkBase[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (chunkBase[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t firstLane(uint64_t mask) { return uint32_t(__builtin_ctzll(mask)); }

__global__ __launch_bounds__(kMatchBlock) void lz4_match_kernel(Lz4Job j) {
    __shared__ uint32_t tables[kMatchBlock / 64][kLz4TableSize];
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(j.scratch);
    if (!H->ok) return;
    const Lz4Layout L = H->L;
    const uint64_t* chunkBase = reinterpret_cast<const uint64_t*>(j.scratch + L.chunkBaseAt);
    const uint64_t* slotBase = reinterpret_cast<const uint64_t*>(j.scratch + L.slotBaseAt);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(j.scratch + L.cntAt);
    uint64_t* lastEndOut = reinterpret_cast<uint64_t*>(j.scratch + L.maxAt);
    Lz4Match* matches = reinterpret_cast<Lz4Match*>(j.scratch + L.matchAt);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* table = tables[wave];
    const uint64_t chunks = H->chunks, stride = uint64_t(gridDim.x) * (kMatchBlock / 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) lastEndOut[chunks] = 0;  // (the scan's last element)
    for (uint64_t c = uint64_t(blockIdx.x) * (kMatchBlock / 64) + wave; c < chunks; c += stride) {
        const uint32_t s = segmentOf(chunkBase, j.nSeg, c);
        const uint64_t k = c - chunkBase[s];
        const uint32_t n = j.segLen[s];
        const uint32_t cb = uint32_t(k * j.C), ce = uint32_t(uint64_t(cb) + j.C < n ? cb + j.C : n);
        const uint8_t* src = j.in + j.segBegin[s];
        Lz4Match* mine = matches + slotBase[s] + k * (j.C / 4);
        uint32_t count = 0, lastEnd = 0;
        uint64_t pos = cb;
        if (lz4TakesPart(pos, ce, n)) {
            for (uint32_t i = lane; i < kLz4TableSize; i += 64) table[i] = 0;
            const uint32_t limit = lz4MatchLimit(ce, n);
            while (lz4TakesPart(pos, ce, n)) {
                const uint64_t p = pos + lane;
                const bool part = lz4TakesPart(p, ce, n);
                uint32_t four = 0, h = 0, e = 0;
                if (part) {
                    four = lz4Load32(src + p);
                    h = lz4Hash(four);
                    e = table[h];
                }
                const bool hit = e != 0 && lz4Load32(src + cb + (e - 1)) == four;
                const uint64_t hits = __ballot(hit);
                const uint32_t f = hits ? firstLane(hits) : 64;
                if (part && lane <= f) atomicMax(&table[h], uint32_t(p - cb) + 1);
                if (!hits) {
                    pos += 64;
                    continue;
                }
                const uint32_t start = uint32_t(pos) + f, from = cb + uint32_t(__shfl(int(e), int(f), 64)) - 1;
                uint32_t len = kLz4MinMatch;
                for (;;) {  // 256 bytes a round: four per lane, the first lane that stops ends the match
                    const uint64_t a = uint64_t(start) + len + 4 * lane;
                    const uint32_t avail = a < limit ? uint32_t(limit - a < 4 ? limit - a : 4) : 0;
                    uint32_t same = 0;
                    if (avail == 4) {
                        const uint32_t x = lz4Load32(src + a) ^ lz4Load32(src + from + len + 4 * lane);
                        same = x ? uint32_t(__builtin_ctz(x)) / 8 : 4;
                    } else {
                        while (same < avail && src[a + same] == src[uint64_t(from) + len + 4 * lane + same]) ++same;
                    }
                    const uint64_t stops = __ballot(same < 4);
                    if (stops) {
                        const uint32_t l2 = firstLane(stops);
                        len += 4 * l2 + uint32_t(__shfl(int(same), int(l2), 64));
                        break;
                    }
                    len += 256;
                }
                if (lane == 0) mine[count] = Lz4Match{start, ((len - kLz4MinMatch) << 16) | (start - from)};
                ++count;
                pos = uint64_t(start) + len;
                lastEnd = start + len;
            }
        }
        if (lane == 0) {
            cnt[c] = count;
            lastEndOut[c] = count ? chunkBase[s] * j.C + lastEnd : 0;  // (in the chunks' own coordinates: they grow from segment to segment)
        }
    }
}

// ---- exclusive scan of v[0 .. chunks + 1) in place, 64-bit; kMax: a running maximum, else a running sum
template <bool kMax>
__device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) {
    return kMax ? (a > b ? a : b) : a + b;
}
template <bool kMax>
__device__ __forceinline__ uint64_t waveInclusiveOp(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= uint32_t(d)) v = join<kMax>(up, v);
    }
    return v;
}

template <bool kMax>
__global__ __launch_bounds__(kBlock) void lz4_scan_sums_kernel(uint8_t* __restrict__ scratch) {
    __shared__ uint64_t waveSums[kBlock / 64];
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(scratch);
    if (!H->ok) return;
    const uint64_t* v = reinterpret_cast<const uint64_t*>(scratch + (kMax ? H->L.maxAt : H->L.sizeAt));
    uint64_t* tileSums = reinterpret_cast<uint64_t*>(scratch + H->L.tileAt);
    const uint64_t m = H->chunks + 1, tiles = lz4Tiles(H->chunks);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t base = tile * kScanTile + threadIdx.x * kScanPerThread;
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t q = 0; q < kScanPerThread; ++q)
            if (base + q < m) acc = join<kMax>(acc, v[base + q]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc = join<kMax>(acc, __shfl_xor((unsigned long long)acc, d, 64));
        if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t total = 0;
            for (uint32_t w = 0; w < kBlock / 64; ++w) total = join<kMax>(total, waveSums[w]);
            tileSums[tile] = total;
        }
        __syncthreads();
    }
}

template <bool kMax>
__global__ __launch_bounds__(kScanTilesPerPass) void lz4_scan_tiles_kernel(uint8_t* __restrict__ scratch) {
    __shared__ uint64_t waveSums[kScanTilesPerPass / 64];
    __shared__ uint64_t carry;
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(scratch);
    if (!H->ok) return;
    uint64_t* tileSums = reinterpret_cast<uint64_t*>(scratch + H->L.tileAt);
    const uint64_t nTiles = lz4Tiles(H->chunks);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t base = 0; base < nTiles; base += kScanTilesPerPass) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t own = i < nTiles ? tileSums[i] : 0;
        const uint64_t incl = waveInclusiveOp<kMax>(own, lane);
        if (lane == 63) waveSums[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before = join<kMax>(before, waveSums[w]);
        // exclusive: what lies in front of tile i -- the carry, the waves in front, the lanes in front
        const uint64_t up = __shfl_up((unsigned long long)incl, 1, 64);
        if (i < nTiles) tileSums[i] = lane ? join<kMax>(before, up) : before;
        __syncthreads();
        if (threadIdx.x == kScanTilesPerPass - 1) carry = join<kMax>(before, incl);
        __syncthreads();
    }
}

template <bool kMax>
__global__ __launch_bounds__(kBlock) void lz4_scan_apply_kernel(uint8_t* __restrict__ scratch) {
    __shared__ uint64_t waveSums[kBlock / 64];
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(scratch);
    if (!H->ok) return;
    uint64_t* v = reinterpret_cast<uint64_t*>(scratch + (kMax ? H->L.maxAt : H->L.sizeAt));
    const uint64_t* tileSums = reinterpret_cast<const uint64_t*>(scratch + H->L.tileAt);
    const uint64_t m = H->chunks + 1, tiles = lz4Tiles(H->chunks);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t base = tile * kScanTile + threadIdx.x * kScanPerThread;
        uint64_t own[kScanPerThread];
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t q = 0; q < kScanPerThread; ++q) {
            own[q] = base + q < m ? v[base + q] : 0;
            acc = join<kMax>(acc, own[q]);
        }
        const uint64_t incl = waveInclusiveOp<kMax>(acc, lane);
        if (lane == 63) waveSums[wave] = incl;
        __syncthreads();
        uint64_t at = tiles > 1 ? tileSums[tile] : 0;  // (one tile: the sums were never made)
        for (uint32_t w = 0; w < wave; ++w) at = join<kMax>(at, waveSums[w]);
        const uint64_t up = __shfl_up((unsigned long long)incl, 1, 64);
        if (lane) at = join<kMax>(at, up);
#pragma unroll
        for (uint32_t q = 0; q < kScanPerThread; ++q) {
            if (base + q < m) v[base + q] = at;
            at = join<kMax>(at, own[q]);
        }
        __syncthreads();
    }
}

// what a wavefront knows of its chunk in the size and emit passes
struct Lz4Chunk {
    uint32_t s, n, count, prevEnd;  // segment, its length, the chunk's matches, the end of the last match in front of the chunk
    bool lastOfSegment;
    const uint8_t* src;
    const Lz4Match* mine;
};
__device__ __forceinline__ Lz4Chunk loadChunk(const Lz4Job& j, const Lz4Head* H, uint64_t c) {
    const Lz4Layout& L = H->L;
    const uint64_t* chunkBase = reinterpret_cast<const uint64_t*>(j.scratch + L.chunkBaseAt);
    const uint64_t* slotBase = reinterpret_cast<const uint64_t*>(j.scratch + L.slotBaseAt);
    Lz4Chunk k;
    k.s = segmentOf(chunkBase, j.nSeg, c);
    const uint64_t first = chunkBase[k.s], inSeg = c - first;
    k.n = j.segLen[k.s];
    k.count = reinterpret_cast<const uint32_t*>(j.scratch + L.cntAt)[c];
    const uint64_t inFront = reinterpret_cast<const uint64_t*>(j.scratch + L.maxAt)[c], origin = first * j.C;
    k.prevEnd = inFront > origin ? uint32_t(inFront - origin) : 0;
    k.lastOfSegment = c + 1 == chunkBase[k.s + 1];
    k.src = j.in + j.segBegin[k.s];
    k.mine = reinterpret_cast<const Lz4Match*>(j.scratch + L.matchAt) + slotBase[k.s] + inSeg * (j.C / 4);
    return k;
}

__global__ __launch_bounds__(kBlock) void lz4_size_kernel(Lz4Job j) {
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(j.scratch);
    if (!H->ok) return;
    uint64_t* sizes = reinterpret_cast<uint64_t*>(j.scratch + H->L.sizeAt);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t chunks = H->chunks, stride = uint64_t(gridDim.x) * (kBlock / 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[chunks] = 0;
    for (uint64_t c = uint64_t(blockIdx.x) * (kBlock / 64) + wave; c < chunks; c += stride) {
        const Lz4Chunk k = loadChunk(j, H, c);
        uint64_t bytes = 0;
        uint32_t anchor = k.prevEnd;
        for (uint32_t i = lane; i < k.count; i += 64) {
            const Lz4Match m = k.mine[i];
            uint32_t before = k.prevEnd;
            if (i) {
                const Lz4Match b = k.mine[i - 1];
                before = b.start + lz4MatchLen(b);
            }
            bytes += lz4SeqSize(m.start - before, lz4MatchLen(m));
        }
        if (k.count) {
            const Lz4Match last = k.mine[k.count - 1];
            anchor = last.start + lz4MatchLen(last);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) bytes += __shfl_xor((unsigned long long)bytes, d, 64);
        if (k.lastOfSegment) bytes += lz4SeqSize(k.n - anchor, 0);
        if (lane == 0) sizes[c] = bytes;
    }
}

// sequence s at out + at, served by lanes sub = 0 .. nl - 1 of a group
__device__ __forceinline__ void writeSeq(uint8_t* __restrict__ out, uint64_t at, const Lz4Seq& s, uint64_t size, uint32_t sub, uint32_t nl) {
    const uint32_t lead = uint32_t((reinterpret_cast<uintptr_t>(out) + at) & 3u);
    uint8_t* base = out + at - lead;  // an aligned word of memory
    const uint64_t end = lead + size;
    for (uint64_t q = uint64_t(sub) * 4; q < end; q += uint64_t(nl) * 4) {
        if (q >= lead && q + 4 <= end) {
            *reinterpret_cast<uint32_t*>(base + q) = lz4SeqWord(s, size, q - lead);
        } else {  // the sequence's first or last partial word: its neighbours own the other bytes
            for (uint32_t b = 0; b < 4; ++b)
                if (q + b >= lead && q + b < end) base[q + b] = lz4SeqByte(s, q + b - lead);
        }
    }
}

template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void lz4_emit_kernel(Lz4Job j, uint8_t* __restrict__ out, uint64_t outCap, uint64_t* __restrict__ outOff,
                                                          uint64_t* __restrict__ totalOut) {
    const Lz4Head* H = reinterpret_cast<const Lz4Head*>(j.scratch);
    if (!H->ok) {  // (the host entries' trips: the refusal goes where the host reads it)
        if (totalOut && blockIdx.x == 0 && threadIdx.x == 0) *totalOut = ~uint64_t(0);
        return;
    }
    const uint64_t* sizes = reinterpret_cast<const uint64_t*>(j.scratch + H->L.sizeAt);
    const uint64_t* chunkBase = reinterpret_cast<const uint64_t*>(j.scratch + H->L.chunkBaseAt);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t chunks = H->chunks, stride = uint64_t(gridDim.x) * (kBlock / 64), total = sizes[chunks];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        outOff[j.nSeg] = total;
        if (totalOut) *totalOut = total;
    }
    const bool room = total <= outCap;  // too small: not one byte of out is stored; the offsets are complete all the same
    constexpr uint32_t kGroups = 64 / kLanes;
    const uint32_t group = lane / kLanes, sub = lane % kLanes;
    for (uint64_t c = uint64_t(blockIdx.x) * (kBlock / 64) + wave; c < chunks; c += stride) {
        const Lz4Chunk k = loadChunk(j, H, c);
        uint64_t at = sizes[c];
        if (lane == 0 && c == chunkBase[k.s]) outOff[k.s] = at;
        if (!room) continue;
        uint32_t anchor = k.prevEnd;
        for (uint32_t first = 0; first < k.count; first += 64) {
            // a lane per sequence: its literals, its size, where it goes
            const uint32_t i = first + lane;
            Lz4Match m{0, 0};
            uint32_t lit = 0;
            uint64_t size = 0;
            if (i < k.count) {
                m = k.mine[i];
                uint32_t before = k.prevEnd;
                if (i) {
                    const Lz4Match b = k.mine[i - 1];
                    before = b.start + lz4MatchLen(b);
                }
                lit = m.start - before;
                size = lz4SeqSize(lit, lz4MatchLen(m));
            }
            const uint64_t incl = waveInclusive(size, lane);
            const uint64_t mineAt = at + incl - size;
            // kLanes lanes per sequence: kGroups sequences a round
#pragma unroll 1
            for (uint32_t r = 0; r < kLanes; ++r) {
                const int from = int(r * kGroups + group);
                const uint32_t start = uint32_t(__shfl(int(m.start), from, 64)), lenOff = uint32_t(__shfl(int(m.lenOff), from, 64));
                const uint32_t l = uint32_t(__shfl(int(lit), from, 64));
                const uint64_t seqAt = __shfl((unsigned long long)mineAt, from, 64), seqSize = __shfl((unsigned long long)size, from, 64);
                if (seqSize == 0) continue;
                const Lz4Match mm{start, lenOff};
                const Lz4Seq s{k.src + (start - l), l, lz4MatchLen(mm), lz4MatchOffset(mm)};
                writeSeq(out, seqAt, s, seqSize, sub, kLanes);
            }
            at += __shfl((unsigned long long)incl, 63, 64);
        }
        if (k.count) {
            const Lz4Match last = k.mine[k.count - 1];
            anchor = last.start + lz4MatchLen(last);
        }
        if (k.lastOfSegment) {  // the closing sequence: the whole wavefront
            const Lz4Seq s{k.src + anchor, k.n - anchor, 0, 0};
            writeSeq(out, at, s, lz4SeqSize(k.n - anchor, 0), lane, 64);
        }
    }
}

}  // namespace lclz4
