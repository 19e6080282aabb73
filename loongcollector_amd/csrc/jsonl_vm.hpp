// jsonl_vm.hpp -- the JSON line of ONE parsed log event, for host and device (include/jsonl/lc_jsonl.h).  Restated from the reference's
// JsonEventGroupSerializer (core/collection_pipeline/serializer/JsonSerializer.cpp:30-84) and rapidjson's Writer::WriteString with its
// default flags:
//
//   record   head decimal(time) { ,"key":" escaped(value) " }... }\n         head = {"k":"v",...,"__time__":  (the group's, lc_jsonl_head)
//   string   " -> \"   \ -> \\   0x08 0x09 0x0A 0x0C 0x0D -> \b \t \n \f \r   every other byte below 0x20 -> \u00XX (upper-case hex)
//            everything else as it is (/, 0x7F, every byte >= 0x80); a string ENDS AT ITS FIRST 0x00 BYTE (the const Ch* overloads)
//   an event that would hold no content writes no record                     e.Empty(), :46
//
// What an event becomes is an item list (JsonlPlanView): item = (the constant bytes `,"<escaped key>":"`, a source); source 0 is the
// whole line, g >= 1 the line's capture group g, of which (-1, -1) is the empty value (itemValue's cut rule is sls_vm.hpp's).
// Shared by host and device:
//   classifyUnit   16 bytes of a value -> masks: which bytes belong to the value, the NULs, the bytes that take two, that take six
//   emitUnit       the escaped bytes of a unit's live bytes at an output position
//   copyPieceLanes a copied piece, lane by lane: a lane owns ALIGNED dwords of the output and assembles each from the source dwords
//                  around it (lcsls::bytes4, the funnel shift); a piece's first and last partial word are byte stores
// How lanes combine units is the kernel's (jsonl_kernel.hpp); jsonlRecordSize / jsonlWriteRecordHost compose the same unit functions
// serially.  Reads: on the device a value is read in aligned 16-byte units that overlap it (the contract for d_data of lc_regex_gpu.h);
// on the host byte by byte, never outside the value.
#pragma once

#include <stdint.h>
#include <string.h>

#include "sls_vm.hpp"

#define LC_JSONL_HD LC_SLS_HD

namespace lcjsonl {

constexpr uint32_t kMaxItems = 256;  // per list
constexpr uint32_t kMaxKeyBytes = 64u << 10;
constexpr uint32_t kMaxHeadBytes = 64u << 10;
constexpr uint32_t kMinHeadBytes = 12;  // {"__time__":
// a record of this size or more is not written (size 0): positions inside a record are 32-bit
constexpr uint64_t kMaxRecordBytes = 0xFFFFFFF0ull;

struct JsonlItem {
    uint32_t prefixAt;   // where in the blob `,"<escaped key>":"` begins (4-byte aligned)
    uint32_t prefixLen;
    uint32_t source;     // 0: the whole line; g >= 1: capture group g
    uint32_t reserved;
};

// items[0 .. nMatched) for a line the parser matched, items[nMatched .. nMatched + nUnmatched) for every other line
struct JsonlPlanView {
    const uint8_t* blob;
    const JsonlItem* items;
    uint32_t nMatched, nUnmatched;
};

struct JsonlEvent {
    const uint8_t* line;
    uint32_t lineLen;
    const int32_t* caps;  // int32[2 * ngroups] of this line
    uint32_t firstItem, nItems;
    uint32_t time;
};

// the value of an item: [*b, *b + *len) of the line.  A row that does not lie inside the line is cut to it.
LC_JSONL_HD void itemValue(const JsonlEvent& e, uint32_t source, uint32_t* b, uint32_t* len) {
    lcsls::SlsEvent s;
    s.lineLen = e.lineLen;
    s.caps = e.caps;
    lcsls::itemValue(s, source, b, len);
}
LC_JSONL_HD void eventItems(const JsonlPlanView& P, uint8_t status, uint32_t* first, uint32_t* count) {
    const bool matched = status == 1;
    *first = matched ? 0 : P.nMatched;
    *count = matched ? P.nMatched : P.nUnmatched;
}

LC_JSONL_HD uint32_t decimalDigits(uint32_t t) {
    uint32_t n = 1;
    while (t >= 10) {
        t /= 10;
        ++n;
    }
    return n;
}
// digit j (0 = the first) of t, which has nd digits
LC_JSONL_HD uint8_t decimalDigit(uint32_t t, uint32_t nd, uint32_t j) {
    for (uint32_t k = j + 1; k < nd; ++k) t /= 10;
    return uint8_t('0' + t % 10);
}

LC_JSONL_HD uint32_t popc32(uint32_t v) { return uint32_t(__builtin_popcount(v)); }
LC_JSONL_HD uint32_t ctz32(uint32_t v) { return uint32_t(__builtin_ctz(v)); }

// ---- one 16-byte unit: bit j of a mask speaks of byte j
struct UnitMasks {
    uint32_t valid;  // bytes that belong to the value
    uint32_t nul;    // ... that are 0x00
    uint32_t two;    // ... that are written as two bytes
    uint32_t six;    // ... that are written as six
};
// 0x80 in every byte of x that is zero (exact: no carry between bytes)
LC_JSONL_HD uint32_t zeroBytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
LC_JSONL_HD uint32_t equalBytes(uint32_t x, uint32_t c) { return zeroBytes(x ^ (c * 0x01010101u)); }
// the four 0x80 flags of a word as bits 0..3
LC_JSONL_HD uint32_t packFlags(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 0xFu; }

// w: the unit as four little-endian words; bytes [lo, hi) of it belong to the value (lo < hi <= 16)
LC_JSONL_HD UnitMasks classifyUnit(const uint32_t w[4], uint32_t lo, uint32_t hi) {
    UnitMasks m;
    m.valid = (0xFFFFu >> (16 - hi)) & (0xFFFFu << lo);
    uint32_t nul = 0, two = 0, ctl = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t x = w[q];
        const uint32_t t = equalBytes(x, '"') | equalBytes(x, '\\') | equalBytes(x, 8) | equalBytes(x, 9) | equalBytes(x, 10) | equalBytes(x, 12) |
                           equalBytes(x, 13);
        nul |= packFlags(zeroBytes(x)) << (4 * q);
        two |= packFlags(t) << (4 * q);
        ctl |= packFlags(zeroBytes(x & 0xE0E0E0E0u)) << (4 * q);
    }
    m.nul = nul & m.valid;
    m.two = two & m.valid;
    m.six = ctl & ~two & ~nul & m.valid;
    return m;
}
// the bytes in front of the unit's first NUL (all valid bytes when it has none)
LC_JSONL_HD uint32_t liveBytes(const UnitMasks& m) { return m.nul ? m.valid & ((1u << ctz32(m.nul)) - 1u) : m.valid; }
LC_JSONL_HD uint32_t escapedBytes(const UnitMasks& m, uint32_t live) { return popc32(live) + popc32(m.two & live) + 5 * popc32(m.six & live); }

LC_JSONL_HD uint8_t hexUpper(uint32_t v) { return uint8_t(v < 10 ? '0' + v : 'A' + (v - 10)); }
// the escaped bytes of the unit's `live` bytes at out[0 ..); returns how many
LC_JSONL_HD uint32_t emitUnit(uint8_t* out, const uint32_t w[4], const UnitMasks& m, uint32_t live) {
    uint32_t p = 0;
    while (live) {
        const uint32_t j = ctz32(live);
        live &= live - 1;
        const uint32_t c = (w[j >> 2] >> (8 * (j & 3u))) & 0xFFu;
        if ((m.two >> j) & 1u) {
            out[p++] = '\\';
            out[p++] = uint8_t(c == 8 ? 'b' : c == 9 ? 't' : c == 10 ? 'n' : c == 12 ? 'f' : c == 13 ? 'r' : c);
        } else if ((m.six >> j) & 1u) {
            out[p++] = '\\';
            out[p++] = 'u';
            out[p++] = '0';
            out[p++] = '0';
            out[p++] = hexUpper(c >> 4);
            out[p++] = hexUpper(c & 15u);
        } else {
            out[p++] = uint8_t(c);
        }
    }
    return p;
}

// src[0 .. len) to out[at .. at + len) as lane `lane` of `lanes` sees it: the lane owns every lanes-th aligned word of the output (out
// itself is 4-byte aligned); a word inside the piece is one 4-byte store, the piece's first and last partial word are byte stores of
// the piece's own bytes, so that the neighbouring pieces' lanes never store the same byte.
LC_JSONL_HD void copyPieceLanes(uint8_t* out, uint64_t at, uint32_t len, const uint8_t* src, uint32_t lane, uint32_t lanes) {
    if (len == 0) return;
    const uint32_t lead = uint32_t(at & 3u);
    uint8_t* base = out + (at - lead);
    const uint64_t end = uint64_t(lead) + len;
    for (uint64_t q = uint64_t(lane) * 4; q < end; q += uint64_t(lanes) * 4) {
        const uint32_t w = lcsls::bytes4(src, len, int64_t(q) - int64_t(lead));
        if (q >= lead && q + 4 <= end) {
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint32_t*>(base + q) = w;
#else
            memcpy(base + q, &w, 4);
#endif
        } else {
            for (uint32_t j = 0; j < 4; ++j)
                if (q + j >= lead && q + j < end) base[q + j] = uint8_t(w >> (8 * j));
        }
    }
}

// ---- the host's serial composition of the unit functions
// a value read byte by byte: its length in front of the first NUL and the escaped length of that
inline void scanValueHost(const uint8_t* v, uint32_t len, uint32_t* rawLen, uint64_t* escLen) {
    uint64_t esc = 0;
    uint32_t raw = len;
    for (uint32_t at = 0; at < len; at += 16) {
        const uint32_t n = len - at < 16 ? len - at : 16;
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n; ++j) w[j >> 2] |= uint32_t(v[at + j]) << (8 * (j & 3u));
        const UnitMasks m = classifyUnit(w, 0, n);
        const uint32_t live = liveBytes(m);
        esc += escapedBytes(m, live);
        if (m.nul) {
            raw = at + popc32(live);
            break;
        }
    }
    *rawLen = raw;
    *escLen = esc;
}
inline uint64_t emitValueHost(uint8_t* out, const uint8_t* v, uint32_t rawLen) {
    uint64_t p = 0;
    for (uint32_t at = 0; at < rawLen; at += 16) {
        const uint32_t n = rawLen - at < 16 ? rawLen - at : 16;
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n; ++j) w[j >> 2] |= uint32_t(v[at + j]) << (8 * (j & 3u));
        const UnitMasks m = classifyUnit(w, 0, n);
        p += emitUnit(out + p, w, m, m.valid);
    }
    return p;
}

// the record's bytes, 0 for no record (no items, or too large)
inline uint64_t jsonlRecordSize(const JsonlPlanView& P, const JsonlEvent& e, uint32_t headLen) {
    if (e.nItems == 0) return 0;
    uint64_t size = uint64_t(headLen) + decimalDigits(e.time) + 2;
    for (uint32_t k = 0; k < e.nItems; ++k) {
        const JsonlItem it = P.items[e.firstItem + k];
        uint32_t b, len, raw;
        uint64_t esc;
        itemValue(e, it.source, &b, &len);
        scanValueHost(e.line + b, len, &raw, &esc);
        size += uint64_t(it.prefixLen) + esc + 1;
        if (size >= kMaxRecordBytes) return 0;
    }
    return size;
}

// The record of one event at out[at .. at + size), size = jsonlRecordSize(...) > 0, piece by piece as the device places them: the copied
// pieces (head, item prefixes, values without a reactive byte) through copyPieceLanes for every lane of `lanes` in turn, the other
// values unit by unit.  out - (at & 3) + at must be 4-byte aligned as on the device.  Touches no byte outside the record.
inline void jsonlWriteRecordHost(const JsonlPlanView& P, const JsonlEvent& e, const uint8_t* head, uint32_t headLen, uint8_t* out, uint64_t at,
                                 uint32_t lanes) {
    uint64_t pos = at;
    for (uint32_t l = 0; l < lanes; ++l) copyPieceLanes(out, pos, headLen, head, l, lanes);
    pos += headLen;
    const uint32_t nd = decimalDigits(e.time);
    for (uint32_t j = 0; j < nd; ++j) out[pos + j] = decimalDigit(e.time, nd, j);
    pos += nd;
    for (uint32_t k = 0; k < e.nItems; ++k) {
        const JsonlItem it = P.items[e.firstItem + k];
        for (uint32_t l = 0; l < lanes; ++l) copyPieceLanes(out, pos, it.prefixLen, P.blob + it.prefixAt, l, lanes);
        pos += it.prefixLen;
        uint32_t b, len, raw;
        uint64_t esc;
        itemValue(e, it.source, &b, &len);
        scanValueHost(e.line + b, len, &raw, &esc);
        if (esc == raw) {
            for (uint32_t l = 0; l < lanes; ++l) copyPieceLanes(out, pos, raw, e.line + b, l, lanes);
        } else {
            emitValueHost(out + pos, e.line + b, raw);
        }
        pos += esc;
        out[pos++] = '"';
    }
    out[pos] = '}';
    out[pos + 1] = '\n';
}

// ---- host only: a string as the reference writes it (cut at its first NUL, escaped), appended to `out` (any container of push_back)
template <class Bytes>
inline void appendEscaped(Bytes& out, const uint8_t* s, size_t len) {
    size_t run = 0, i = 0;  // s[run .. i): bytes that are copied as they are
    for (; i < len; ++i) {
        const uint8_t c = s[i];
        if (c >= 0x20 && c != '"' && c != '\\') continue;
        out.insert(out.end(), s + run, s + i);
        if (c == 0) return;
        uint32_t w[4] = {c, 0, 0, 0};
        const UnitMasks m = classifyUnit(w, 0, 1);
        uint8_t tmp[6];
        const uint32_t n = emitUnit(tmp, w, m, m.valid);
        out.insert(out.end(), tmp, tmp + n);
        run = i + 1;
    }
    out.insert(out.end(), s + run, s + i);
}

}  // namespace lcjsonl
