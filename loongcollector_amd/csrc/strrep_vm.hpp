// strrep_vm.hpp -- the per-value routines of the string-replace processor (include/strrep/lc_strrep.h), ONE set of functions for the
// host and the device, for the size pass (a sink that counts) and the write pass (a sink that stores).
//
// Both methods are walked 16-byte unit by 16-byte unit, left to right, in "tile coordinates" (position 0 is the 16-byte boundary at or
// below the value's first byte, the value occupies [head, head + len), as in anchor_vm.hpp and kv_vm.hpp).  A unit OWNS the pieces of
// output that START in it: a literal byte, a selected occurrence of Match (const), a decode unit -- a raw byte, an escape, a UTF-8
// sequence -- of the unquote.  What a piece needs behind its unit's end (the rest of a needle, an escape's digits, continuation bytes)
// is read through the source's byteAt(); what it covers there is the NEXT unit's "skip":
//   const    strrepConstUnit     cover: the tile position up to which the bytes belong to an occurrence selected earlier.  One 16-bit
//                                mask of the bytes that equal Match's first byte (the quad-mask idiom of anchor_vm.hpp), cut to the
//                                positions at or behind the cover and inside the value; the needle's further bytes are confirmed only at
//                                set bits; a confirmed occurrence moves the cover behind itself, which is strings.ReplaceAll's greedy
//                                left-to-right selection (a candidate inside the cover is never looked at: `aa` on `aaaaa`).
//   unquote  strrepUnquoteUnit   a cursor (p, v): raw position p, and in form B, where a raw `"` IS the four units `\`, `x`, `2`, `2`,
//                                how many of the four are consumed (v).  strrepDecodeOne is strconv.UnquoteChar over that unit stream.
// The size pass records per unit (bytes its pieces produce, skip at its entry): strrepRecord.  The write pass gives every unit to a lane,
// which starts from the recorded skip and needs nothing from its neighbours but a prefix sum of the byte counts.
#pragma once

#include <stdint.h>

#include "../../include/strrep/lc_strrep.h"

#if defined(__HIPCC__)
#define LC_STRREP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_STRREP_HD inline
#endif

enum : uint32_t { kStrrepConst = 0, kStrrepUnquote = 1 };

// what lc_strrep_create fixes; passed to the kernels by value and copied to LDS once per workgroup (the lanes index the needle and the
// replacement with their own positions)
struct StrrepConfig {
    uint8_t match[LC_STRREP_MAX_MATCH];
    uint8_t repl[LC_STRREP_MAX_REPLACE];
    uint32_t method, matchLen, replLen, pad;
};
constexpr uint32_t kStrrepReplAt = LC_STRREP_MAX_MATCH;  // where repl begins in the table
static_assert(sizeof(StrrepConfig) % 16 == 0, "copied to LDS as words");

// a unit's record: the bytes its pieces produce (const: at most 16 * 256) and the skip at its entry (const: cover - unit begin, below 48;
// unquote: (p - unit begin) << 2 | v, at most (16 << 2) for a form A value whose opening quote is a unit's last byte)
LC_STRREP_HD uint32_t strrepRecord(uint32_t bytes, uint32_t skip) { return bytes | (skip << 24); }
LC_STRREP_HD uint32_t strrepRecordBytes(uint32_t r) { return r & 0xFFFFFFu; }
LC_STRREP_HD uint32_t strrepRecordSkip(uint32_t r) { return r >> 24; }

// one bit per byte of the quad q (bit j = byte j) that equals the byte spread over b4 (anchor_vm.hpp's anchorEqQuad, restated)
LC_STRREP_HD uint32_t strrepEqNibble(uint32_t x, uint32_t b4) {
    const uint32_t y = x ^ b4;
    const uint32_t u = (~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) >> 7;
    return (u | (u >> 7) | (u >> 14) | (u >> 21)) & 0xFu;
}
LC_STRREP_HD uint32_t strrepEqQuad(const uint32_t q[4], uint32_t b4) {
    return strrepEqNibble(q[0], b4) | (strrepEqNibble(q[1], b4) << 4) | (strrepEqNibble(q[2], b4) << 8) | (strrepEqNibble(q[3], b4) << 12);
}
// the bits lo .. hi - 1 of a quad's mask (0 <= lo, hi <= 16)
LC_STRREP_HD uint32_t strrepBitRange(uint32_t lo, uint32_t hi) { return lo >= hi ? 0u : ((0xFFFFu << lo) & 0xFFFFu) & (0xFFFFu >> (16 - hi)); }

// ------------------------------------------------------------------------------------------------ const
// The unit [ub, ub + 16) of a value that ends at tile position `end`; q: the unit's 16 bytes; *cover: in, where the walk stands (>= ub for
// every unit but one the cover reaches over entirely); out, where it stands behind the unit's pieces (>= min(ub + 16, end)).
// Sink: void lit(const Source&, uint32_t p0, uint32_t p1) -- the bytes [p0, p1) go out as they are; void repl() -- ReplaceString goes out.
// Returns the occurrences that start in the unit.
template <class Bytes, class Source, class Sink>
LC_STRREP_HD uint32_t strrepConstUnit(Bytes match, uint32_t m, const uint32_t q[4], uint32_t ub, uint32_t end, uint32_t* cover, const Source& src, Sink& sink) {
    const uint32_t upper = end - ub < 16 ? end : ub + 16;
    uint32_t p = *cover;
    if (p >= upper) return 0;
    // a candidate's last byte must lie inside the value: first bytes at or behind end - m + 1 are no candidates
    const uint32_t lastStart = end >= m ? end - m + 1 : 0;  // (exclusive)
    const uint32_t hiBit = lastStart <= ub ? 0u : lastStart - ub < 16 ? lastStart - ub : 16u;
    uint32_t mask = strrepEqQuad(q, uint32_t(match[0]) * 0x01010101u) & strrepBitRange(p - ub, hiBit);
    uint32_t found = 0;
    while (mask) {
        const uint32_t at = ub + uint32_t(__builtin_ctz(mask));
        mask &= mask - 1;
        if (at < p) continue;  // inside the cover of an occurrence selected in this unit
        bool same = true;
        for (uint32_t j = 1; j < m && same; ++j) same = src.byteAt(at + j) == match[j];
        if (!same) continue;
        sink.lit(src, p, at);
        sink.repl();
        p = at + m;
        ++found;
    }
    if (p < upper) {
        sink.lit(src, p, upper);
        p = upper;
    }
    *cover = p;
    return found;
}

// ------------------------------------------------------------------------------------------------ unquote
struct StrrepCursor {
    uint32_t p, v;     // raw tile position; form B: units of the `"` at p already consumed (0..3)
    uint32_t error;    // the decode failed
    uint32_t escaped;  // a backslash escape was decoded or a byte became EF BF BD
};

// the next byte of the unit stream, or -1 at vend (the value's end: an escape may read the closing quote of form A, never behind it)
template <class Source>
LC_STRREP_HD int32_t strrepNext(const Source& src, bool formB, uint32_t vend, StrrepCursor* c) {
    if (c->p >= vend) return -1;
    const uint32_t b = src.byteAt(c->p);
    if (formB && b == '"') {
        const uint32_t v = c->v;
        if (v == 3) {
            c->v = 0;
            ++c->p;
        } else {
            c->v = v + 1;
        }
        return v == 0 ? '\\' : v == 1 ? 'x' : '2';
    }
    ++c->p;
    return int32_t(b);
}

LC_STRREP_HD int32_t strrepHex(int32_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// how many bytes the well-formed UTF-8 sequence at p takes (2..4), by Go's utf8 tables; 0: there is none (b0 >= 0x80 is the byte at p;
// cend: where the content ends -- a byte behind it is no continuation byte in either form)
template <class Source>
LC_STRREP_HD uint32_t strrepUtf8(const Source& src, uint32_t b0, uint32_t p, uint32_t cend) {
    uint32_t need, lo = 0x80, hi = 0xBF;
    if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
    else if (b0 >= 0xE0 && b0 <= 0xEF) need = 3, lo = b0 == 0xE0 ? 0xA0 : 0x80, hi = b0 == 0xED ? 0x9F : 0xBF;
    else if (b0 >= 0xF0 && b0 <= 0xF4) need = 4, lo = b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xF4 ? 0x8F : 0xBF;
    else return 0;
    if (cend - p < need) return 0;
    for (uint32_t j = 1; j < need; ++j) {
        const uint32_t b = src.byteAt(p + j);
        if (b < lo || b > hi) return 0;
        lo = 0x80, hi = 0xBF;
    }
    return need;
}

template <class Sink>
LC_STRREP_HD void strrepPutRune(Sink& sink, uint32_t r) {
    if (r < 0x80) {
        sink.put(r);
    } else if (r < 0x800) {
        sink.put(0xC0 | (r >> 6));
        sink.put(0x80 | (r & 0x3F));
    } else if (r < 0x10000) {
        sink.put(0xE0 | (r >> 12));
        sink.put(0x80 | ((r >> 6) & 0x3F));
        sink.put(0x80 | (r & 0x3F));
    } else {
        sink.put(0xF0 | (r >> 18));
        sink.put(0x80 | ((r >> 12) & 0x3F));
        sink.put(0x80 | ((r >> 6) & 0x3F));
        sink.put(0x80 | (r & 0x3F));
    }
}

// one decode unit at the cursor (c->p < cend): strconv.UnquoteChar(s, '"') and the caller's loop around it (strconv/quote.go, Go 1.23).
// Sink: void put(uint32_t byte).
template <class Source, class Sink>
LC_STRREP_HD void strrepDecodeOne(const Source& src, bool formB, uint32_t cend, uint32_t vend, StrrepCursor* c, Sink& sink) {
    if (formB && c->v == 0 && src.byteAt(c->p) == '"') {  // `\x22`, whole: the quote itself, and nothing to flag
        sink.put('"');
        ++c->p;
        return;
    }
    const uint32_t at = c->p;
    const int32_t b = strrepNext(src, formB, vend, c);
    if (b == '"' || b == '\n') {  // (form A: an unescaped quote in front of the last byte)
        c->error = 1;
        return;
    }
    if (b >= 0x80) {
        const uint32_t n = strrepUtf8(src, uint32_t(b), at, cend);
        if (n == 0) {
            sink.put(0xEF);
            sink.put(0xBF);
            sink.put(0xBD);
            c->escaped = 1;
            return;
        }
        sink.put(uint32_t(b));
        for (uint32_t j = 1; j < n; ++j) sink.put(src.byteAt(at + j));
        c->p = at + n;
        return;
    }
    if (b != '\\') {
        sink.put(uint32_t(b));
        return;
    }
    c->escaped = 1;
    const int32_t e = strrepNext(src, formB, vend, c);
    uint32_t digits = 0;
    switch (e) {
        case 'a': sink.put(7); return;
        case 'b': sink.put(8); return;
        case 'f': sink.put(12); return;
        case 'n': sink.put(10); return;
        case 'r': sink.put(13); return;
        case 't': sink.put(9); return;
        case 'v': sink.put(11); return;
        case '\\': sink.put('\\'); return;
        case '"': sink.put('"'); return;
        case 'x': digits = 2; break;
        case 'u': digits = 4; break;
        case 'U': digits = 8; break;
        default:
            if (e >= '0' && e <= '7') {
                uint32_t val = uint32_t(e - '0');
                for (uint32_t j = 0; j < 2; ++j) {
                    const int32_t d = strrepNext(src, formB, vend, c);
                    if (d < '0' || d > '7') {
                        c->error = 1;
                        return;
                    }
                    val = (val << 3) | uint32_t(d - '0');
                }
                if (val > 255) c->error = 1;
                else sink.put(val);
                return;
            }
            c->error = 1;  // \' , the input's end, everything else
            return;
    }
    uint32_t val = 0;
    for (uint32_t j = 0; j < digits; ++j) {
        const int32_t h = strrepHex(strrepNext(src, formB, vend, c));
        if (h < 0) {
            c->error = 1;
            return;
        }
        val = (val << 4) | uint32_t(h);  // (eight digits fill the word exactly: nothing is lost before the range check)
    }
    if (digits == 2) {
        sink.put(val);  // the RAW byte
        return;
    }
    if (val > 0x10FFFFu || (val >= 0xD800u && val <= 0xDFFFu)) {
        c->error = 1;
        return;
    }
    strrepPutRune(sink, val);
}

// The value's shape: form A (begins and ends with `"`) or B; where its content begins and ends.  False: the one-byte value `"`, an error.
struct StrrepShape {
    bool formB;
    uint32_t cbegin, cend, vend;  // content [cbegin, cend); escapes read up to vend
};
LC_STRREP_HD bool strrepShape(uint32_t head, uint32_t len, uint32_t firstByte, uint32_t lastByte, StrrepShape* s) {
    const uint32_t end = head + len;
    const bool formA = len != 0 && firstByte == '"' && lastByte == '"';
    s->formB = !formA;
    s->vend = end;
    s->cbegin = formA ? head + 1 : head;
    s->cend = formA ? end - 1 : end;
    return !(formA && len < 2);
}

// every decode unit that starts in [max(ub, cursor), min(ub + 16, cend))
template <class Source, class Sink>
LC_STRREP_HD void strrepUnquoteUnit(const Source& src, const StrrepShape& s, uint32_t ub, StrrepCursor* c, Sink& sink) {
    const uint32_t upper = s.cend - ub < 16 || s.cend < ub ? s.cend : ub + 16;
    while (c->p < upper && !c->error) strrepDecodeOne(src, s.formB, s.cend, s.vend, c, sink);
}
// behind the value's last unit: the closing quote stands where the content ends (form A: `\` in front of it, or an escape that read
// it as a digit and failed already; form B: always, the quote is the appended one)
LC_STRREP_HD bool strrepUnquoteClosed(const StrrepShape& s, const StrrepCursor& c) { return !c.error && c.p == s.cend && c.v == 0; }

// ------------------------------------------------------------------------------------------------ the host's walk
// a byte pointer as the source; the value lies `head` bytes behind a 16-byte boundary.  Bytes outside the value read as Match's first
// byte (const) or a backslash (unquote): the walk must not take them for the value's
struct StrrepHostSource {
    const uint8_t* line;
    uint32_t len, head;
    uint8_t junk;
    uint32_t byteAt(uint32_t p) const { return p >= head && p - head < len ? line[p - head] : junk; }
    void quad(uint32_t ub, uint32_t q[4]) const {
        for (int t = 0; t < 4; ++t) q[t] = 0;
        for (uint32_t j = 0; j < 16; ++j) q[j >> 2] |= byteAt(ub + j) << ((j & 3) * 8);
    }
};
struct StrrepCountSink {
    uint32_t bytes = 0, replLen = 0;
    template <class Source>
    LC_STRREP_HD void lit(const Source&, uint32_t p0, uint32_t p1) { bytes += p1 - p0; }
    LC_STRREP_HD void repl() { bytes += replLen; }
    LC_STRREP_HD void put(uint32_t) { ++bytes; }
};
template <class Bytes>
struct StrrepStoreSink {
    uint8_t* out;
    uint8_t* limit;  // nothing is stored at or behind it
    Bytes replBytes;
    uint32_t replLen;
    LC_STRREP_HD void put(uint32_t b) {
        if (out < limit) *out = uint8_t(b);
        ++out;
    }
    template <class Source>
    LC_STRREP_HD void lit(const Source& src, uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < p1; ++p) put(src.byteAt(p));
    }
    LC_STRREP_HD void repl() {
        for (uint32_t j = 0; j < replLen; ++j) put(replBytes[j]);
    }
};

// The size pass of one value on the host, unit by unit as the kernel walks it: *flags, the output length (0 without CHANGED), and the
// units' records (records: room for (head + len + 15) / 16 words, or null).
inline uint64_t strrepSizeHost(const StrrepConfig& cfg, const uint8_t* line, uint32_t len, uint32_t head, uint8_t* flags, uint32_t* records) {
    head &= 15u;
    const uint32_t end = head + len, units = (end + 15) / 16;
    StrrepHostSource src{line, len, head, cfg.method == kStrrepConst ? cfg.match[0] : uint8_t('\\')};
    uint64_t total = 0;
    *flags = 0;
    if (cfg.method == kStrrepConst) {
        uint32_t cover = head, found = 0;
        for (uint32_t u = 0; u < units && len; ++u) {
            uint32_t q[4];
            src.quad(u * 16, q);
            StrrepCountSink sink;
            sink.replLen = cfg.replLen;
            const uint32_t skip = cover > u * 16 ? cover - u * 16 : 0;
            found += strrepConstUnit(cfg.match, cfg.matchLen, q, u * 16, end, &cover, src, sink);
            if (records) records[u] = strrepRecord(sink.bytes, skip);
            total += sink.bytes;
        }
        if (found) *flags = LC_STRREP_CHANGED;
        return found ? total : 0;
    }
    StrrepShape s;
    if (!strrepShape(head, len, len ? line[0] : 0, len ? line[len - 1] : 0, &s)) {
        *flags = LC_STRREP_ERROR;
        return 0;
    }
    StrrepCursor c{s.cbegin, 0, 0, 0};
    for (uint32_t u = 0; u < units && len; ++u) {
        StrrepCountSink sink;
        const uint32_t skip = c.p > u * 16 || c.v ? ((c.p - u * 16) << 2) | c.v : 0;
        strrepUnquoteUnit(src, s, u * 16, &c, sink);
        if (records) records[u] = strrepRecord(sink.bytes, skip);
        total += sink.bytes;
    }
    if (!strrepUnquoteClosed(s, c)) {
        *flags = LC_STRREP_ERROR;
        return 0;
    }
    if (!s.formB || c.escaped) *flags = LC_STRREP_CHANGED;
    return *flags ? total : 0;
}

// The write pass of one CHANGED value on the host: every unit on its own, from its record alone, in ANY order (here: last unit first),
// as the kernel's lanes do.  out: room for exactly the size pass's length.
inline void strrepWriteHost(const StrrepConfig& cfg, const uint8_t* line, uint32_t len, uint32_t head, const uint32_t* records, uint8_t* out, uint64_t outLen) {
    head &= 15u;
    const uint32_t end = head + len, units = (end + 15) / 16;
    StrrepHostSource src{line, len, head, cfg.method == kStrrepConst ? cfg.match[0] : uint8_t('\\')};
    StrrepShape s{};
    if (cfg.method == kStrrepUnquote) strrepShape(head, len, len ? line[0] : 0, len ? line[len - 1] : 0, &s);
    for (uint32_t u = units; u-- > 0;) {
        uint64_t at = 0;
        for (uint32_t k = 0; k < u; ++k) at += strrepRecordBytes(records[k]);
        const uint32_t bytes = strrepRecordBytes(records[u]), skip = strrepRecordSkip(records[u]);
        if (!bytes) continue;
        StrrepStoreSink<const uint8_t*> sink{out + at, out + (at + bytes < outLen ? at + bytes : outLen), cfg.repl, cfg.replLen};
        if (cfg.method == kStrrepConst) {
            uint32_t q[4], cover = u * 16 + skip;
            src.quad(u * 16, q);
            strrepConstUnit(cfg.match, cfg.matchLen, q, u * 16, end, &cover, src, sink);
        } else {
            StrrepCursor c{u * 16 + (skip >> 2), skip & 3u, 0, 0};
            strrepUnquoteUnit(src, s, u * 16, &c, sink);
        }
    }
}
