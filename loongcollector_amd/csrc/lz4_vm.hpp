// lz4_vm.hpp -- the rules of the LZ4 block writer (include/lz4/lc_lz4.h), once for the host and the device.  lz4_kernel.hpp runs them
// with one wavefront per chunk; lz4CompressHost() below restates the wavefront as a loop over 64 lanes and is what the device is held
// to, bit for bit (tests/native/lz4_host_check.cpp runs it stand-alone).
//
// A segment of n bytes becomes ONE LZ4 block (block format, no frame).  What a decoder-side check may rely on:
//   chunks     The segment is cut into chunks of C bytes (64 <= C <= 65536, a multiple of 64); chunk k is [kC, min((k + 1)C, n)).  A
//              match and its source lie inside ONE chunk: every offset is 1 .. C - 1, no match crosses a multiple of C, matches never
//              overlap and stand in ascending order.  A literal run may span any number of chunks.
//   end rules  a match starts at or before n - 12 and ends at or before n - 5 (LZ4's own); a segment below 13 bytes has no match
//   a step     at `pos` (a chunk starts with pos = its begin and an EMPTY table of kLz4TableSize entries): lane l = 0..63 looks at
//              p = pos + l and takes part iff p + 4 <= the chunk's end and p <= n - 12.  It reads the table entry of lz4Hash(the four
//              bytes at p) AS IT WAS BEFORE THE STEP; a hit is an entry that names a position q whose four bytes equal those at p (q lies
//              in front of pos and inside the chunk, because only earlier steps of this chunk stored it).  f = the lowest lane with a hit.
//                no hit   every lane that takes part stores its position; pos += 64
//                a hit    the lanes <= f that take part store their positions (the lanes behind f do NOT: storing them costs ratio, and
//                         storing before the read would let a position meet itself); the match starts at pos + f, its length is the
//                         common prefix of the bytes at q and at pos + f, cut at min(the chunk's end, n - 5); pos = start + length
//              the chunk ends at the first step in which lane 0 does not take part (then no lane does)
//   the table  an entry is position - chunk begin + 1 (0: empty).  Several lanes that store into one entry in a step leave the HIGHEST
//              position (the device: an LDS atomic max; positions only grow from step to step, so a max over all time is the same).
//   the bytes  the matches of all chunks in order are the block's sequences: token, literal length bytes (15 + 255k), literals, offset
//              (2 bytes LE), match length bytes on length - 4; a closing sequence of the literals behind the last match (token and
//              length bytes only; at least 5 literals when the block has a match); n = 0 is the one byte 00.
//              A block never exceeds lz4Bound(n) = n + n / 255 + 16.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LC_LZ4_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_LZ4_HD inline
#endif

namespace lclz4 {

constexpr uint32_t kLz4TableBits = 12;
constexpr uint32_t kLz4TableSize = 1u << kLz4TableBits;  // 4096 x 4 B = 16 KiB of LDS per wavefront
constexpr uint32_t kLz4MinChunk = 64, kLz4MaxChunk = 65536;
constexpr uint32_t kLz4SegLimit = 0x7E000000u;           // a segment is shorter than this (LZ4_MAX_INPUT_SIZE)
constexpr uint32_t kLz4MinMatch = 4, kLz4LastLiterals = 5, kLz4MatchFindLimit = 12;

LC_LZ4_HD uint32_t lz4Load32(const uint8_t* p) {  // (any alignment; the four bytes are the caller's to read)
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
LC_LZ4_HD uint32_t lz4Hash(uint32_t four) { return (four * 2654435761u) >> (32 - kLz4TableBits); }

LC_LZ4_HD uint64_t lz4Bound(uint64_t n) { return n + n / 255 + 16; }

// does position p of a chunk that ends at chunkEnd, in a segment of n bytes, take part in a step?
LC_LZ4_HD bool lz4TakesPart(uint64_t p, uint32_t chunkEnd, uint32_t n) { return p + 4 <= chunkEnd && p + kLz4MatchFindLimit <= n; }
// where a match of this chunk ends at the latest (only asked when a lane took part, so n >= 12)
LC_LZ4_HD uint32_t lz4MatchLimit(uint32_t chunkEnd, uint32_t n) { return chunkEnd < n - kLz4LastLiterals ? chunkEnd : n - kLz4LastLiterals; }

// a match as the match pass records it: start relative to the SEGMENT, length, offset
struct Lz4Match {
    uint32_t start;
    uint32_t lenOff;  // (length - 4) << 16 | offset: both fit 16 bits, the chunk is at most 65536 bytes
};
LC_LZ4_HD uint32_t lz4MatchLen(const Lz4Match& m) { return (m.lenOff >> 16) + kLz4MinMatch; }
LC_LZ4_HD uint32_t lz4MatchOffset(const Lz4Match& m) { return m.lenOff & 0xFFFFu; }

// the length bytes of a run of v (15 + 255k): how many there are
LC_LZ4_HD uint32_t lz4LenBytes(uint32_t v) { return v < 15 ? 0 : (v - 15) / 255 + 1; }
// a sequence's size: lit literals and a match of matchLen; matchLen 0 = the closing sequence
LC_LZ4_HD uint64_t lz4SeqSize(uint32_t lit, uint32_t matchLen) {
    const uint64_t head = 1 + uint64_t(lz4LenBytes(lit)) + lit;
    return matchLen ? head + 2 + lz4LenBytes(matchLen - kLz4MinMatch) : head;
}

// One sequence for the emit pass: byte j of it (0 <= j < size).  src points at the sequence's first literal.
struct Lz4Seq {
    const uint8_t* src;
    uint32_t lit, matchLen, offset;  // matchLen 0: the closing sequence
};
LC_LZ4_HD uint8_t lz4LenByte(uint32_t v, uint32_t j) {  // byte j of the length bytes of v >= 15
    const uint32_t count = (v - 15) / 255 + 1;
    return j + 1 < count ? 255 : uint8_t((v - 15) % 255);
}
LC_LZ4_HD uint8_t lz4SeqByte(const Lz4Seq& s, uint64_t j) {
    const uint32_t ml = s.matchLen ? s.matchLen - kLz4MinMatch : 0;
    if (j == 0) return uint8_t(((s.lit < 15 ? s.lit : 15) << 4) | (ml < 15 ? ml : 15));
    const uint32_t le = lz4LenBytes(s.lit);
    if (j <= le) return lz4LenByte(s.lit, uint32_t(j - 1));
    const uint64_t litAt = 1 + uint64_t(le);
    if (j < litAt + s.lit) return s.src[j - litAt];
    const uint64_t k = j - litAt - s.lit;
    if (k == 0) return uint8_t(s.offset);
    if (k == 1) return uint8_t(s.offset >> 8);
    return lz4LenByte(ml, uint32_t(k - 2));
}
// the four bytes j .. j + 3 of the sequence (a byte at or behind `size` reads as 0); a word inside the literals is one load
LC_LZ4_HD uint32_t lz4SeqWord(const Lz4Seq& s, uint64_t size, uint64_t j) {
    const uint64_t litAt = 1 + uint64_t(lz4LenBytes(s.lit));
    if (j >= litAt && j + 4 <= litAt + s.lit) return lz4Load32(s.src + (j - litAt));
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b)
        if (j + b < size) w |= uint32_t(lz4SeqByte(s, j + b)) << (8 * b);
    return w;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---------------------------------------------------------------------------------------------------------------- the host routine
// The matches of chunk [cb, ce) of src[0..n), appended to `out` (start relative to the segment): the wavefront as a loop over lanes.
// table: kLz4TableSize words, the caller's; emptied here.
template <class Out>
inline void lz4ChunkMatchesHost(const uint8_t* src, uint32_t n, uint32_t cb, uint32_t ce, uint32_t* table, Out* out) {
    for (uint32_t i = 0; i < kLz4TableSize; ++i) table[i] = 0;
    uint64_t pos = cb;
    while (lz4TakesPart(pos, ce, n)) {
        uint32_t cand[64];
        bool part[64];
        uint32_t f = 64;
        for (uint32_t l = 0; l < 64; ++l) {  // every lane reads the table as it was before the step
            const uint64_t p = pos + l;
            part[l] = lz4TakesPart(p, ce, n);
            cand[l] = 0;
            if (!part[l]) continue;
            const uint32_t four = lz4Load32(src + p);
            const uint32_t e = table[lz4Hash(four)];
            if (e && lz4Load32(src + cb + (e - 1)) == four) {
                cand[l] = e;
                if (f == 64) f = l;
            }
        }
        for (uint32_t l = 0; l < 64 && l <= f; ++l) {  // the lanes <= f store; the highest position stays
            if (!part[l]) continue;
            const uint32_t rel = uint32_t(pos + l - cb) + 1;
            uint32_t& slot = table[lz4Hash(lz4Load32(src + pos + l))];
            if (rel > slot) slot = rel;
        }
        if (f == 64) {
            pos += 64;
            continue;
        }
        const uint32_t start = uint32_t(pos) + f, from = cb + (cand[f] - 1), limit = lz4MatchLimit(ce, n);
        uint32_t len = kLz4MinMatch;
        while (start + len < limit && src[from + len] == src[start + len]) ++len;
        out->push_back(Lz4Match{start, ((len - kLz4MinMatch) << 16) | (start - from)});
        pos = uint64_t(start) + len;
    }
}

// src[0..n) as one block into out (room for lz4Bound(n)); returns the block's size.  chunk: C.  Written byte by byte, apart from the
// device's word assembly (lz4SeqWord), so that the two check each other.
template <class Vec>
inline uint64_t lz4CompressHost(const uint8_t* src, uint32_t n, uint32_t chunk, uint8_t* out, Vec* matches) {
    uint32_t table[kLz4TableSize];
    matches->clear();
    for (uint64_t cb = 0; cb < n; cb += chunk) lz4ChunkMatchesHost(src, n, uint32_t(cb), uint32_t(cb + chunk < n ? cb + chunk : n), table, matches);
    uint64_t at = 0;
    uint32_t anchor = 0;
    auto putLen = [&](uint32_t v) {
        if (v < 15) return;
        v -= 15;
        for (; v >= 255; v -= 255) out[at++] = 255;
        out[at++] = uint8_t(v);
    };
    for (const Lz4Match& m : *matches) {
        const uint32_t lit = m.start - anchor, ml = lz4MatchLen(m) - kLz4MinMatch, off = lz4MatchOffset(m);
        out[at++] = uint8_t(((lit < 15 ? lit : 15) << 4) | (ml < 15 ? ml : 15));
        putLen(lit);
        for (uint32_t i = 0; i < lit; ++i) out[at++] = src[anchor + i];
        out[at++] = uint8_t(off);
        out[at++] = uint8_t(off >> 8);
        putLen(ml);
        anchor = m.start + lz4MatchLen(m);
    }
    const uint32_t lit = n - anchor;
    out[at++] = uint8_t((lit < 15 ? lit : 15) << 4);
    putLen(lit);
    for (uint32_t i = 0; i < lit; ++i) out[at++] = src[anchor + i];
    return at;
}
#endif

}  // namespace lclz4
