// anchor_vm.hpp -- the per-value routine of the anchor processor, ONE function for the host and the device.
//
// anchorLocate() does for one value what ProcessorAnchor.ProcessAnchor does (plugins/processor/anchor/anchor.go :172-199) before it
// touches the log: per anchor the first Start, then the first Stop at or behind Start's end, reported as a span.  The Go searches the
// value twice per anchor (up to 32 searches from byte 0 for 16 anchors); this routine makes ONE forward pass for all anchors together:
//   * an anchor is in one of three phases: Start is looked for; Stop is looked for, from begin on; resolved.  (What is still open at
//     the value's end is "no start" / "no stop".)
//   * per 16-byte quad and per open anchor: one 16-bit mask of the bytes that equal the FIRST byte of the needle the anchor is looking
//     for (Start's or Stop's, chosen per lane by a select between two wave-uniform bytes), cut to the bits at or behind the anchor's own
//     lower bound and inside the value, a jump to the first set bit, the needle's further bytes confirmed only there (byteAt: the needle
//     may straddle a quad, a stage, the tile).  A candidate whose last byte would lie behind the value's end is no occurrence.
//   * when a Start is confirmed, the SAME quad is examined again for the anchor's Stop, from begin on: Start and Stop inside one
//     quad and an empty field are ordinary cases.  A Stop's lower bound is begin, never Start's first byte: an occurrence that
//     overlaps Start's tail does not count.
//   * an empty Start gives begin = 0 before the walk, an empty Stop end = len the moment Start is known: an empty needle is never
//     searched for.
//   * an anchor that no lane of the wavefront has open is skipped by a wave-uniform test, and a wavefront without an open anchor in
//     any lane that still has bytes stops fetching stages (anchors usually sit near the front of a line).
// Per-lane state is no array: the phases are packed into one word, a begin / end goes to the lane's own result row the moment it is
// known, and what the Stop search needs of begin is one byte per anchor (see anchorLocate).
//
// The routine never touches memory itself: the bytes come from a SOURCE (template parameter), the one of kv_vm.hpp -- 16-byte quads
// in "tile coordinates": position 0 is the 16-byte boundary at or below the value's first byte, the value occupies [head, head + len):
//
//   struct Source {
//       uint32_t head() const;                          // 0..15
//       uint32_t stageCount(uint32_t end);              // 64-byte stages to walk for a value that ends at tile position end (0: none);
//                                                       //   the device answers for the whole WAVEFRONT (the stage loop is uniform)
//       void stage(uint32_t s);                         // make stage s current (the device: cooperative load into the LDS tile)
//       void rowQuad(uint32_t k, uint32_t q[4]);        // quad k (0..3) of the current stage of THIS value
//       uint32_t byteAt(uint32_t p) const;              // the byte at tile position p, head <= p < head + len
//   };
//
// The host source (AnchorHostSource below) answers the positions behind the value with the bytes that FOLLOW it in a packed buffer
// (given apart, so that the value itself stays an exactly-sized block) and everything else with needle first bytes.
#pragma once

#include <stdint.h>

#include "../../include/anchor/lc_anchor.h"

#if defined(__HIPCC__)
#define LC_ANCHOR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_ANCHOR_HD inline
#endif

constexpr uint32_t kAnchorStageBytes = 64;

// what lc_anchor_create fixes; passed to the kernel by value (constant kernel arguments); the first kAnchorTableBytes are copied to LDS
// once per workgroup
struct AnchorConfig {
    uint8_t start[LC_ANCHOR_MAX_ANCHORS][LC_ANCHOR_MAX_NEEDLE];
    uint8_t stop[LC_ANCHOR_MAX_ANCHORS][LC_ANCHOR_MAX_NEEDLE];
    // per anchor what a quad's visit needs, in one word: Start's first byte, Stop's first byte, len(Start), len(Stop) (0..32)
    uint32_t meta[LC_ANCHOR_MAX_ANCHORS];
    uint32_t count;  // 0..16
};
constexpr uint32_t kAnchorNeedleBytes = 2 * LC_ANCHOR_MAX_ANCHORS * LC_ANCHOR_MAX_NEEDLE;
constexpr uint32_t kAnchorTableBytes = kAnchorNeedleBytes + 4 * LC_ANCHOR_MAX_ANCHORS;

// entries per row: the count rounded up to an even number
inline uint32_t anchorStride(const AnchorConfig& c) { return (c.count + 1u) & ~1u; }

// false: a needle above its bound, or no room for another anchor
inline bool anchorAdd(AnchorConfig* c, const uint8_t* start, size_t sl, const uint8_t* stop, size_t pl) {
    if (c->count >= LC_ANCHOR_MAX_ANCHORS || sl > LC_ANCHOR_MAX_NEEDLE || pl > LC_ANCHOR_MAX_NEEDLE) return false;
    const uint32_t a = c->count++;
    for (size_t i = 0; i < sl; ++i) c->start[a][i] = start[i];
    for (size_t i = 0; i < pl; ++i) c->stop[a][i] = stop[i];
    c->meta[a] = uint32_t(c->start[a][0]) | (uint32_t(c->stop[a][0]) << 8) | (uint32_t(sl) << 16) | (uint32_t(pl) << 24);
    return true;
}

// true if any lane of the wavefront says so (the host: the one value there is)
LC_ANCHOR_HD bool anchorWaveAny(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(x) != 0;
#else
    return x;
#endif
}

// one bit per byte of the quad q (bit j = byte j) that equals the byte spread over b4.  Per dword: bit 7 of every equal byte (exact: no
// carry crosses a byte), then the four bits 7, 15, 23, 31 drawn together.
LC_ANCHOR_HD uint32_t anchorEqNibble(uint32_t x, uint32_t b4) {
    const uint32_t y = x ^ b4;
    const uint32_t u = (~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) >> 7;  // bits 0, 8, 16, 24
    return (u | (u >> 7) | (u >> 14) | (u >> 21)) & 0xFu;
}
LC_ANCHOR_HD uint32_t anchorEqQuad(const uint32_t q[4], uint32_t b4) {
    return anchorEqNibble(q[0], b4) | (anchorEqNibble(q[1], b4) << 4) | (anchorEqNibble(q[2], b4) << 8) | (anchorEqNibble(q[3], b4) << 12);
}
// the bits lo .. hi - 1 of a quad's mask (lo, hi: any integers; clamped to 0..16)
LC_ANCHOR_HD uint32_t anchorBitRange(int32_t lo, int32_t hi) {
    const uint32_t below = lo <= 0 ? 0xFFFFu : lo >= 16 ? 0u : (0xFFFFu << lo) & 0xFFFFu;
    const uint32_t above = hi >= 16 ? 0xFFFFu : hi <= 0 ? 0u : (1u << hi) - 1u;
    return below & above;
}

// needle[1 .. nlen) at value position pos + 1 ..; the caller has checked pos + nlen <= len and the first byte
template <class Source, class Bytes>
LC_ANCHOR_HD bool anchorMatch(const Source& src, uint32_t head, Bytes needle, uint32_t nlen, uint32_t pos) {
    for (uint32_t j = 1; j < nlen; ++j)
        if (src.byteAt(head + pos + j) != needle[j]) return false;
    return true;
}

// one of four words by a wave-uniform index: selects over a scalar condition, nothing is indexed in memory
LC_ANCHOR_HD uint32_t anchorPick(uint32_t i, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) { return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : w3; }

enum : uint32_t { kAnchorSeekStart = 0, kAnchorSeekStop = 1, kAnchorResolved = 2 };

// Sink: void begin(uint32_t a, int32_t b), void end(uint32_t a, int32_t e) -- entry a's two numbers, each stored the moment it is known;
// void none(uint32_t a, int32_t code) -- entry a is (code, -1).  table, meta: the needle bytes and the per-anchor words wherever the
// lanes read them from, laid out as AnchorConfig's first two arrays and its meta array; Bytes / Words are pointers to uint8_t / uint32_t
// (the host: into the config itself; the device: into LDS, in LDS's address space, so that a read is an LDS read and not a flat one);
// every lane reads the same address, so what it reads is wave-uniform.  count: the configured anchors (wave-uniform).
// Per-lane state: the phases, two bits per anchor, in one word; per anchor one byte "the lower bound of my search, counted from the
// base of the next quad I look at" (0 .. 31: the value's head in the first quad, what is left of a Start that reaches over a quad's end),
// four to a word.  A begin is stored to the row when Start is confirmed and never read again: the Stop search needs only the byte.
template <class Bytes, class Words, class Source, class Sink>
LC_ANCHOR_HD void anchorLocate(Bytes table, Words meta, uint32_t count, Source& src, Sink& sink, uint32_t len) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;  // tile position
    uint32_t ph = 0;
    uint32_t w0 = head * 0x01010101u, w1 = w0, w2 = w0, w3 = w0;
#pragma unroll 1
    for (uint32_t a = 0; a < count; ++a) {
        const uint32_t w = meta[a];
        if (((w >> 16) & 0xFFu) != 0) continue;
        sink.begin(a, 0);  // Index(val, "") = 0
        if ((w >> 24) == 0) sink.end(a, int32_t(len));
        ph |= ((w >> 24) == 0 ? kAnchorResolved : kAnchorSeekStop) << (2 * a);
    }
    const uint32_t doneMask = uint32_t((uint64_t(1) << (2 * count)) - 1) & 0xAAAAAAAAu;
    bool open = (ph & doneMask) != doneMask;  // an anchor of this value is
    const uint32_t stages = src.stageCount(open && len != 0 ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        const uint32_t base = s * kAnchorStageBytes;
        if (!anchorWaveAny(open && base < end)) break;  // nothing left to find in this wavefront: the rest is not fetched
        src.stage(s);
#pragma unroll 1
        for (uint32_t k = 0; k < kAnchorStageBytes / 16; ++k) {
            const uint32_t qbase = base + k * 16;
            const bool walking = open && qbase < end;
            if (!anchorWaveAny(walking)) break;  // (a value ends once: no later quad of the stage has a walking lane)
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll 1
            for (uint32_t a = 0; a < count; ++a) {
                const uint32_t phase = (ph >> (2 * a)) & 3u;
                const bool mine = walking && phase != kAnchorResolved;
                if (!anchorWaveAny(mine)) continue;  // no lane has this anchor open
                if (mine) {
                    const uint32_t sh = (a & 3u) * 8;
                    int32_t lo = int32_t((anchorPick(a >> 2, w0, w1, w2, w3) >> sh) & 0xFFu);  // the lower bound, as a bit of this quad
                    const uint32_t w = meta[a];
                    const uint32_t s4 = (w & 0xFFu) * 0x01010101u, p4 = ((w >> 8) & 0xFFu) * 0x01010101u;
                    const uint32_t sl = (w >> 16) & 0xFFu, pl = w >> 24;
                    bool stopPhase = phase == kAnchorSeekStop;
                    uint32_t mask = anchorEqQuad(q, stopPhase ? p4 : s4);
                    for (;;) {
                        const uint32_t m = mask & anchorBitRange(lo, int32_t(end) - int32_t(qbase));
                        if (!m) break;
                        const uint32_t j = uint32_t(__builtin_ctz(m));
                        const uint32_t pos = qbase + j - head;
                        const uint32_t nlen = stopPhase ? pl : sl;
                        const Bytes needle = table + ((stopPhase ? kAnchorNeedleBytes / 2 : 0u) + a * LC_ANCHOR_MAX_NEEDLE);
                        lo = int32_t(j) + 1;
                        if (pos + nlen <= len && anchorMatch(src, head, needle, nlen, pos)) {
                            if (stopPhase) {
                                sink.end(a, int32_t(pos));
                                ph = (ph & ~(3u << (2 * a))) | (kAnchorResolved << (2 * a));
                                break;
                            }
                            sink.begin(a, int32_t(pos + nlen));
                            if (pl == 0) {  // Index(val[b:], "") = 0, and :190-191
                                sink.end(a, int32_t(len));
                                ph |= kAnchorResolved << (2 * a);
                                break;
                            }
                            ph |= kAnchorSeekStop << (2 * a);
                            stopPhase = true;
                            mask = anchorEqQuad(q, p4);  // the same quad again, for Stop, from begin on
                            lo = int32_t(j + sl);
                        }
                    }
                    const uint32_t next = lo > 16 ? uint32_t(lo - 16) : 0u, clear = ~(0xFFu << sh), put = next << sh;
                    const uint32_t i = a >> 2;
                    w0 = i == 0 ? (w0 & clear) | put : w0;
                    w1 = i == 1 ? (w1 & clear) | put : w1;
                    w2 = i == 2 ? (w2 & clear) | put : w2;
                    w3 = i == 3 ? (w3 & clear) | put : w3;
                }
            }
            open = walking && (ph & doneMask) != doneMask;
        }
        // (a lane that did not walk the stage's last quads keeps `open` as the quad loop left it: false once its value has ended)
    }
    const uint32_t S = (count + 1u) & ~1u;
#pragma unroll 1
    for (uint32_t a = 0; a < S; ++a) {
        const uint32_t phase = a < count ? (ph >> (2 * a)) & 3u : kAnchorSeekStart;  // (the pad entry of an odd count: -1, -1)
        if (phase != kAnchorResolved) sink.none(a, phase == kAnchorSeekStop ? LC_ANCHOR_NO_STOP : LC_ANCHOR_NO_START);
    }
}

// the host's source: a byte pointer; a position behind the value reads the bytes that follow it in a packed buffer (`tail`), every other
// byte outside the value as a needle's first byte
struct AnchorHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    const uint8_t* tail;
    uint32_t tailLen;
    uint8_t junk[2 * LC_ANCHOR_MAX_ANCHORS];
    AnchorHostSource(const uint8_t* l, uint32_t n, uint32_t head, const AnchorConfig& c, const uint8_t* t = nullptr, uint32_t tn = 0)
        : line(l), len(n), headBytes(head & 15u), tail(t), tailLen(tn) {
        for (uint32_t a = 0; a < LC_ANCHOR_MAX_ANCHORS; ++a) {
            const uint32_t k = c.count ? a % c.count : 0;
            junk[2 * a] = c.count && ((c.meta[k] >> 16) & 0xFFu) ? c.start[k][0] : uint8_t(':');
            junk[2 * a + 1] = c.count && (c.meta[k] >> 24) ? c.stop[k][0] : uint8_t('\t');
        }
    }
    uint32_t head() const { return headBytes; }
    uint32_t byteAt(uint32_t p) const {
        if (p >= headBytes && p < headBytes + len) return line[p - headBytes];
        if (p >= headBytes + len && p - headBytes - len < tailLen) return tail[p - headBytes - len];
        return junk[p % (2 * LC_ANCHOR_MAX_ANCHORS)];
    }
    uint32_t stageCount(uint32_t end) const { return (end + kAnchorStageBytes - 1) / kAnchorStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kAnchorStageBytes + k * 16;
        for (int t = 0; t < 4; ++t) q[t] = 0;
        for (uint32_t j = 0; j < 16; ++j) q[j >> 2] |= byteAt(p16 + j) << ((j & 3) * 8);
    }
};

struct AnchorHostSink {
    int32_t* row;  // int32[S][2]
    void begin(uint32_t a, int32_t b) { row[2 * a] = b; }
    void end(uint32_t a, int32_t e) { row[2 * a + 1] = e; }
    void none(uint32_t a, int32_t code) { row[2 * a] = code, row[2 * a + 1] = -1; }
};

// one value on the host, placed `head` bytes behind a 16-byte boundary; row: int32[anchorStride(c)][2]
inline void anchorLocateHost(const AnchorConfig& c, const uint8_t* line, uint32_t len, uint32_t head, int32_t* row, const uint8_t* tail = nullptr,
                             uint32_t tailLen = 0) {
    AnchorHostSource src(line, len, head, c, tail, tailLen);
    AnchorHostSink sink{row};
    anchorLocate(&c.start[0][0], &c.meta[0], c.count, src, sink, len);
}
