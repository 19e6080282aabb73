// kv_vm.hpp -- the per-value routine of the key-value splitter, ONE function for the host and the device.
//
// kvSplitLine() does for one value what KeyValueSplitter.splitKeyValue does (plugins/processor/split/keyvalue/key_value_splitter.go
// :99-143, with concatQuotePair :145-158, getNearestQuote :160-182 and getValue :184-192) before it touches the log: it finds the pairs
// and reports them as spans.  The Go searches each remainder three times (the delimiter, the separator inside the pair,
// Separator+Quote) and restarts its ` \Q` search from every skipped quote; this routine makes ONE forward pass:
//   * NORMAL phase, pair begins at b: the first Delimiter at or behind b ends the pair; on the way the first Separator and the first
//     Separator+Quote behind b are noted.  An occurrence that does not lie wholly inside the pair is no occurrence of the pair (and
//     since it is the first one, none lies inside): that is checked when the pair's end is known.
//   * the extension test of concatQuotePair is made at the delimiter: suffix and prefix by looking at the pair's own bytes, the
//     `Index(pair, Separator+Quote) > 0` from the noted position (an occurrence AT b makes it false, later ones or not).
//   * EXT phase (the pair is extended): only the quote's first byte (and the separator's, while the pair has none) is looked for.  A
//     one-byte quote at p is skipped if and only if p >= start + 2 and the two bytes before it are a space and a backslash -- that is
//     what `lastQuoteContent + 1 == lastQuote` comes to, because the FIRST quote behind the start is the quote of the FIRST ` \Q` or
//     of none -- and the search goes on from p + 1, which looks at quotes from p + 2 on.  No look-back needs a backslash in the mask.
//   * no closing quote: the pair ends one byte behind where the (last) search began (one byte quote) or where :177 says (longer
//     quotes), and the Go splits on from there -- bytes this pass has already walked.  There is then no quote left behind that point, so
//     what remains is a plain split: the routine walks the stages once more from the new pair's first byte.  That second walk can
//     never end in a third.
// A position behind the value's end from :177 is LC_KV_REF_PANIC (the Go's `content[:dIdx]` panics there).
// Three forms (template parameter QM): no quote; a one-byte quote, where every quote byte is an event in both phases and the tests above
// read the walk's notes instead of the value's bytes (events come in position order and a one-byte needle cannot overlap itself, so the
// notes are exact); a longer quote, where those tests compare bytes.
//
// The routine never touches memory itself: the bytes come from a SOURCE (template parameter) that hands out 16-byte quads in "tile
// coordinates" -- position 0 is the 16-byte boundary at or below the value's first byte, the value occupies [head, head + len):
//
//   struct Source {
//       uint32_t head() const;                          // 0..15
//       uint32_t stageCount(uint32_t end);              // 64-byte stages to walk for a value that ends at tile position end (0: none);
//                                                       //   the device answers for the whole WAVEFRONT (the stage loop is uniform)
//       void stage(uint32_t s);                         // make stage s current (the device: cooperative load into the LDS tile)
//       void rowQuad(uint32_t k, uint32_t q[4]);        // quad k (0..3) of the current stage of THIS value
//       uint32_t byteAt(uint32_t p) const;              // the byte at tile position p, head <= p < head + len: a needle's further
//                                                       //   bytes and the look-backs (a needle may straddle a quad, a stage, the tile)
//   };
//
// Per quad the routine builds one 16-bit mask per needle (the bytes that equal its first byte), jumps to the first set bit of the masks
// the current phase cares about and confirms longer needles only there (the quad skip).
// The host source (KvHostSource below) returns delimiter, separator, quote and backslash bytes for everything outside the value.
#pragma once

#include <stdint.h>

#include "../../include/kvsplit/lc_kvsplit.h"

#if defined(__HIPCC__)
#define LC_KV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_KV_HD inline
#endif

constexpr uint32_t kKvStageBytes = 64;
constexpr uint32_t kKvNone = 0xFFFFFFFFu;

// what lc_kvsplit_create fixes; passed to the kernel by value (constant kernel arguments), copied to LDS once per workgroup
struct KvConfig {
    uint8_t delim[LC_KV_MAX_NEEDLE], sep[LC_KV_MAX_NEEDLE], quote[LC_KV_MAX_NEEDLE];
    uint32_t delimLen, sepLen, quoteLen;  // 1..32, 1..32, 0..32
};

// false: a needle outside its bounds
inline bool kvMakeConfig(const uint8_t* d, size_t dl, const uint8_t* s, size_t sl, const uint8_t* q, size_t ql, KvConfig* out) {
    if (dl < 1 || dl > LC_KV_MAX_NEEDLE || sl < 1 || sl > LC_KV_MAX_NEEDLE || ql > LC_KV_MAX_NEEDLE) return false;
    KvConfig c{};
    for (size_t i = 0; i < dl; ++i) c.delim[i] = d[i];
    for (size_t i = 0; i < sl; ++i) c.sep[i] = s[i];
    for (size_t i = 0; i < ql; ++i) c.quote[i] = q[i];
    c.delimLen = uint32_t(dl), c.sepLen = uint32_t(sl), c.quoteLen = uint32_t(ql);
    *out = c;
    return true;
}

// the needles as the routine reads them: the bytes wherever they live (the host: the config; the device: LDS), lengths and the first
// bytes spread over a word
struct KvNeedles {
    const uint8_t *delim, *sep, *quote;
    uint32_t delimLen, sepLen, quoteLen;
    uint32_t d4, s4, q4;
};
LC_KV_HD KvNeedles kvNeedles(const uint8_t* bytes /* a KvConfig's three arrays */, uint32_t dl, uint32_t sl, uint32_t ql, uint32_t d0, uint32_t s0,
                             uint32_t q0) {
    return KvNeedles{bytes, bytes + LC_KV_MAX_NEEDLE, bytes + 2 * LC_KV_MAX_NEEDLE, dl, sl, ql, d0 * 0x01010101u, s0 * 0x01010101u, q0 * 0x01010101u};
}

enum : uint32_t { kKvNormal = 0, kKvExt = 1, kKvDone = 2 };
enum : uint32_t { kKvBitD = 1, kKvBitS = 2, kKvBitQ = 4 };
// the three forms of the routine (template parameter QM): no quote -- no extension logic at all; a one-byte quote -- every quote byte is an
// event in both phases and the suffix / prefix / Separator+Quote / getValue tests read the walk's own notes; a longer quote -- the quote
// is looked for in the EXT phase only and those tests compare the bytes
enum : int { kKvQuoteNone = 0, kKvQuoteOne = 1, kKvQuoteLong = 2 };

struct KvWalk {
    uint32_t b = 0;             // the current pair's first byte
    uint32_t cur = 0;           // the next position to look at
    uint32_t sepPos = kKvNone;  // the first Separator at or behind b
    uint32_t sqPos = kKvNone;   // the first Separator+Quote at or behind b (NORMAL phase)
    uint32_t sp = 0, minQ = 0;  // EXT phase: getNearestQuote's startPos; the first position a quote may begin at
    // one-byte quote (kKvQuoteOne): what the pair's quotes have shown so far, so that no test has to read a byte again
    uint32_t lastQEnd = kKvNone;    // the end of the latest quote at or behind b
    uint32_t lastSepEnd = kKvNone;  // the end of the latest separator (a one-byte separator only)
    bool qAtB = false, qAfterSep = false;  // a quote at b; a quote right behind the first separator
    uint32_t phase = kKvNormal;
    uint32_t npairs = 0, nNoSep = 0, nEmpty = 0;
    uint32_t status = LC_KV_OK;
    bool again = false;         // the stages are walked once more, from cur
};

// one bit per byte of the quad q (bit j = byte j) that equals the byte spread over b4.  Per dword: bit 7 of every equal byte (exact: no
// carry crosses a byte), then the four bits 7, 15, 23, 31 drawn together.
LC_KV_HD uint32_t kvEqNibble(uint32_t x, uint32_t b4) {
    const uint32_t y = x ^ b4;
    const uint32_t u = (~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) >> 7;  // bits 0, 8, 16, 24
    return (u | (u >> 7) | (u >> 14) | (u >> 21)) & 0xFu;
}
LC_KV_HD uint32_t kvEqQuad(const uint32_t q[4], uint32_t b4) {
    return kvEqNibble(q[0], b4) | (kvEqNibble(q[1], b4) << 4) | (kvEqNibble(q[2], b4) << 8) | (kvEqNibble(q[3], b4) << 12);
}
// the bits lo .. hi - 1 of a quad's mask (lo, hi: any integers; clamped to 0..16)
LC_KV_HD uint32_t kvBitRange(int32_t lo, int32_t hi) {
    const uint32_t below = lo <= 0 ? 0xFFFFu : lo >= 16 ? 0u : (0xFFFFu << lo) & 0xFFFFu;
    const uint32_t above = hi >= 16 ? 0xFFFFu : hi <= 0 ? 0u : (1u << hi) - 1u;
    return below & above;
}

// needle[from .. nlen) at value position pos; the caller has checked pos + nlen <= len
template <class Source>
LC_KV_HD bool kvMatch(const Source& src, uint32_t head, const uint8_t* needle, uint32_t nlen, uint32_t from, uint32_t pos) {
    for (uint32_t j = from; j < nlen; ++j)
        if (src.byteAt(head + pos + j) != needle[j]) return false;
    return true;
}

template <int QM, class Source, class Sink>
LC_KV_HD void kvEmit(const KvNeedles& nd, const Source& src, Sink& sink, KvWalk& w, uint32_t head, uint32_t e) {
    const bool hasSep = w.sepPos != kKvNone && w.sepPos + nd.sepLen <= e;  // :112
    uint32_t vb = hasSep ? w.sepPos + nd.sepLen : w.b, ve = e;
    if (QM == kKvQuoteOne) {  // getValue :184-192 from the notes: every quote up to e has been an event
        if (ve - vb >= 2 && (hasSep ? w.qAfterSep : w.qAtB) && w.lastQEnd == e) vb += 1, ve -= 1;
    } else if (QM == kKvQuoteLong) {
        const uint32_t ql = nd.quoteLen;
        if (ve - vb >= 2 * ql && kvMatch(src, head, nd.quote, ql, 0, vb) && kvMatch(src, head, nd.quote, ql, 0, ve - ql)) vb += ql, ve -= ql;
    }
    // (selects and sums, no branch that picks which counter to touch: the walk's state stays in registers)
    const bool noSep = !hasSep, emptyKey = hasSep && w.sepPos == w.b;  // :113-123, :127-129
    const int32_t kb = noSep ? LC_KV_NO_SEPARATOR : emptyKey ? LC_KV_EMPTY_KEY : int32_t(w.b);
    const int32_t ke = int32_t(noSep ? w.nNoSep : emptyKey ? w.nEmpty : w.sepPos);
    w.nNoSep += noSep ? 1u : 0u;
    w.nEmpty += emptyKey ? 1u : 0u;
    sink.pair(w.npairs, kb, ke, int32_t(vb), int32_t(ve));
    ++w.npairs;
}

LC_KV_HD void kvStartPair(KvWalk& w, uint32_t at) {
    w.b = w.cur = at;
    w.sepPos = w.sqPos = w.lastQEnd = w.lastSepEnd = kKvNone;
    w.qAtB = w.qAfterSep = false;
    w.phase = kKvNormal;
}

// the extended pair ends at e (:152-155), and the loop's step behind it (:137-141)
template <int QM, class Source, class Sink>
LC_KV_HD void kvFinishExt(const KvNeedles& nd, const Source& src, Sink& sink, KvWalk& w, uint32_t head, uint32_t len, uint32_t e) {
    kvEmit<QM>(nd, src, sink, w, head, e);
    if (e + nd.delimLen > len) w.phase = kKvDone;
    else kvStartPair(w, e + nd.delimLen);  // the len(Delimiter) bytes behind the pair are skipped whatever they are
}

// `Index(pair, Separator+Quote) > 0` for the pair [b, pos): the first occurrence behind b lies wholly inside the pair and NOT at b
LC_KV_HD bool kvSepQuoteAboveZero(const KvWalk& w, uint32_t needleLen, uint32_t pos) {
    return w.sqPos != kKvNone && w.sqPos > w.b && w.sqPos + needleLen <= pos;
}

// a byte at value position pos whose flag bits (kKvBit*) the phase asked for
template <int QM, class Source, class Sink>
LC_KV_HD void kvEvent(const KvNeedles& nd, const Source& src, Sink& sink, KvWalk& w, uint32_t head, uint32_t len, uint32_t pos, uint32_t bits) {
    w.cur = pos + 1;
    if (w.phase == kKvNormal && (bits & kKvBitD) && pos + nd.delimLen <= len && kvMatch(src, head, nd.delim, nd.delimLen, 1, pos)) {  // :103
        bool extend = false;
        if (QM == kKvQuoteOne) {  // :148-149 from the notes (a quote AT pos is not part of the pair and has not been noted yet)
            if (w.lastQEnd != pos) extend = kvSepQuoteAboveZero(w, nd.sepLen + 1, pos) || w.qAtB;
        } else if (QM == kKvQuoteLong) {
            const uint32_t ql = nd.quoteLen, plen = pos - w.b;
            const bool suffix = plen >= ql && kvMatch(src, head, nd.quote, ql, 0, pos - ql);
            if (!suffix) {
                extend = kvSepQuoteAboveZero(w, nd.sepLen + ql, pos);
                if (!extend) extend = plen >= ql && kvMatch(src, head, nd.quote, ql, 0, w.b);
            }
        }
        if (!extend) {
            kvEmit<QM>(nd, src, sink, w, head, pos);
            kvStartPair(w, pos + nd.delimLen);
            return;
        }
        w.phase = kKvExt;
        w.sp = pos;
        w.minQ = pos + 1;  // Index(content[startPos+1:], Quote)
    }
    if (QM == kKvQuoteOne && (bits & kKvBitQ)) {  // the notes; before the separator's: Separator+Quote wants the separator that ENDS here
        if (w.phase == kKvNormal && w.sqPos == kKvNone && w.lastSepEnd == pos) w.sqPos = pos - 1;
        w.lastQEnd = pos + 1;
        if (pos == w.b) w.qAtB = true;
        if (w.sepPos != kKvNone && pos == w.sepPos + nd.sepLen) w.qAfterSep = true;
    }
    if ((bits & kKvBitS) && (w.sepPos == kKvNone || (QM != kKvQuoteNone && w.phase == kKvNormal && w.sqPos == kKvNone)) && pos + nd.sepLen <= len &&
        kvMatch(src, head, nd.sep, nd.sepLen, 1, pos)) {
        if (w.sepPos == kKvNone) w.sepPos = pos;
        if (QM == kKvQuoteOne && nd.sepLen == 1) {
            w.lastSepEnd = pos + 1;  // (the quote's event at pos + 1 makes it Separator+Quote)
        } else if (QM != kKvQuoteNone && w.phase == kKvNormal && w.sqPos == kKvNone && pos + nd.sepLen + nd.quoteLen <= len &&
                   kvMatch(src, head, nd.quote, nd.quoteLen, 0, pos + nd.sepLen)) {
            w.sqPos = pos;
        }
    }
    if (QM != kKvQuoteNone && w.phase == kKvExt && (bits & kKvBitQ) && pos >= w.minQ && pos + nd.quoteLen <= len && kvMatch(src, head, nd.quote, nd.quoteLen, 1, pos)) {
        uint32_t e;
        if (QM == kKvQuoteOne) {  // :163-175
            if (pos >= w.sp + 2 && src.byteAt(head + pos - 2) == ' ' && src.byteAt(head + pos - 1) == '\\') {
                w.sp = pos + 1;  // `continue`: the loop's test, then quotes from startPos + 1 on
                w.minQ = pos + 2;
                if (w.sp >= len) kvFinishExt<QM>(nd, src, sink, w, head, len, len);
                return;
            }
            e = pos + 1;
        } else {  // :177
            e = pos - 1 + nd.sepLen + nd.quoteLen;
            if (e > len) {
                w.status = LC_KV_REF_PANIC;
                w.phase = kKvDone;
                return;
            }
            // the separator may first occur behind the quote's first byte and still inside the pair: bytes this walk would only see
            // once the next pair has begun
            for (uint32_t t = pos + 1; w.sepPos == kKvNone && t + nd.sepLen <= e; ++t)
                if (kvMatch(src, head, nd.sep, nd.sepLen, 0, t)) w.sepPos = t;
        }
        kvFinishExt<QM>(nd, src, sink, w, head, len, e);
    }
}

// Sink: void pair(uint32_t k, int32_t kb, int32_t ke, int32_t vb, int32_t ve) -- row k of the value (the sink drops k >= W)
template <int QM, class Source, class Sink>
LC_KV_HD void kvSplitLine(const KvNeedles& nd, Source& src, Sink& sink, uint32_t len, uint8_t* statusOut, uint32_t* npairsOut) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;  // tile position
    KvWalk w;
    bool first = true;
    for (;;) {
        // the first walk: every value that has bytes; a further one: only the values that have to go back (a quote form)
        const uint32_t stages = src.stageCount((first ? len != 0 : w.again) ? end : 0u);
        if (!first && stages == 0) break;
        const bool walking = first || w.again;
        first = w.again = false;
        for (uint32_t s = 0; s < stages; ++s) {
            src.stage(s);
            const uint32_t base = s * kKvStageBytes;
            if (!walking || w.phase == kKvDone || base >= end || base + kKvStageBytes <= head + w.cur) continue;
#pragma unroll 1
            for (uint32_t k = 0; k < kKvStageBytes / 16; ++k) {
                const uint32_t qbase = base + k * 16;
                if (w.phase == kKvDone || qbase >= end || qbase + 16 <= head + w.cur) continue;
                uint32_t q[4];
                src.rowQuad(k, q);
                const uint32_t mD = kvEqQuad(q, nd.d4), mS = kvEqQuad(q, nd.s4), mQ = QM != kKvQuoteNone ? kvEqQuad(q, nd.q4) : 0u;
                for (;;) {  // the quad skip: straight to the next byte this phase cares about
                    uint32_t m = 0;
                    if (w.phase == kKvNormal) m |= mD;
                    if (w.phase != kKvDone && (w.sepPos == kKvNone || (QM != kKvQuoteNone && w.phase == kKvNormal && w.sqPos == kKvNone))) m |= mS;
                    if (QM != kKvQuoteNone && (w.phase == kKvExt || (QM == kKvQuoteOne && w.phase == kKvNormal))) m |= mQ;
                    m &= kvBitRange(int32_t(head + w.cur) - int32_t(qbase), int32_t(end) - int32_t(qbase));
                    if (!m) break;
                    const uint32_t j = uint32_t(__builtin_ctz(m));
                    const uint32_t bits = ((mD >> j) & 1u) | (((mS >> j) & 1u) << 1) | (((mQ >> j) & 1u) << 2);
                    kvEvent<QM>(nd, src, sink, w, head, len, qbase + j - head, bits);
                }
            }
        }
        if (!walking) continue;
        // ---- the value's end
        if (w.phase == kKvNormal) {  // :105-106: no delimiter, the pair is the rest (it may be empty)
            kvEmit<QM>(nd, src, sink, w, head, len);
            w.phase = kKvDone;
        } else if (QM != kKvQuoteNone && w.phase == kKvExt) {  // no closing quote
            const uint32_t e = QM == kKvQuoteOne ? w.sp + 1 : w.sp - 1 + nd.sepLen + nd.quoteLen;  // :166 with lastQuote = -1 / :177
            if (e > len) {
                w.status = LC_KV_REF_PANIC;
                w.phase = kKvDone;
            } else {
                kvFinishExt<QM>(nd, src, sink, w, head, len, e);
                if (w.phase == kKvNormal) {
                    if (w.cur == len) {  // nothing left but the empty pair
                        kvEmit<QM>(nd, src, sink, w, head, len);
                        w.phase = kKvDone;
                    } else {
                        w.again = true;
                    }
                }
            }
        }
        if (QM == kKvQuoteNone) break;
    }
    *statusOut = uint8_t(w.status);
    *npairsOut = w.npairs;
}

// the host's source: a byte pointer; every byte outside the value reads as one of four bytes the routine would react to
struct KvHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    uint8_t junk[4];
    KvHostSource(const uint8_t* l, uint32_t n, uint32_t head, const KvConfig& c) : line(l), len(n), headBytes(head & 15u) {
        junk[0] = c.delim[0], junk[1] = c.sep[0], junk[2] = c.quoteLen ? c.quote[0] : uint8_t('"'), junk[3] = '\\';
    }
    uint32_t head() const { return headBytes; }
    uint32_t byteAt(uint32_t p) const { return (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : junk[p & 3u]; }
    uint32_t stageCount(uint32_t end) const { return (end + kKvStageBytes - 1) / kKvStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kKvStageBytes + k * 16;
        for (int t = 0; t < 4; ++t) q[t] = 0;
        for (uint32_t j = 0; j < 16; ++j) q[j >> 2] |= byteAt(p16 + j) << ((j & 3) * 8);
    }
};

struct KvHostSink {
    int32_t* rows;  // int32[W][4]
    uint32_t W;
    void pair(uint32_t k, int32_t kb, int32_t ke, int32_t vb, int32_t ve) {
        if (k < W) rows[k * 4] = kb, rows[k * 4 + 1] = ke, rows[k * 4 + 2] = vb, rows[k * 4 + 3] = ve;
    }
};

// one value on the host, placed `head` bytes behind a 16-byte boundary
inline void kvSplitLineHost(const KvConfig& c, const uint8_t* line, uint32_t len, uint32_t head, int32_t* rows, uint32_t W, uint8_t* status, uint32_t* npairs) {
    const KvNeedles nd = kvNeedles(c.delim, c.delimLen, c.sepLen, c.quoteLen, c.delim[0], c.sep[0], c.quote[0]);
    KvHostSource src(line, len, head, c);
    KvHostSink sink{rows, W};
    if (c.quoteLen > 1) kvSplitLine<kKvQuoteLong>(nd, src, sink, len, status, npairs);
    else if (c.quoteLen == 1) kvSplitLine<kKvQuoteOne>(nd, src, sink, len, status, npairs);
    else kvSplitLine<kKvQuoteNone>(nd, src, sink, len, status, npairs);
}
