// sls_vm.hpp -- the SLS LogGroup wire bytes of ONE parsed log event, for host and device (include/sls/lc_sls.h).  Restated from the
// reference's hand-rolled writer (core/protobuf/sls/LogGroupSerializer.cpp) and the two passes of SLSEventGroupSerializer
// (core/collection_pipeline/serializer/SLSSerializer.cpp:254-268, :377-395):
//
//   content     0x12 varint(S(klen) + S(vlen)) 0x0A varint(klen) key 0x12 varint(vlen) value      AddLogContent :122-137
//   log record  0x0A varint(logSZ) 0x08 varint5(max(time, 2^28)) content... [0x25 fixed32le(ns)]    StartToAddLog / AddLogTime /
//                                                                                                   AddLogTimeNs :105-143
//   S(x) = 1 + varint_size(x) + x;  logSZ = sum of the content sizes + 6 (+ 5 with ns)              GetLogSize :234-248
//   an event that would hold no content writes no record                                            e.Empty(), SLSSerializer.cpp:260, :383
//
// What an event becomes is an item list (SlsPlanView): item = (the constant bytes `0x0A varint(klen) key 0x12`, a source); source 0 is
// the whole line, g >= 1 the line's capture group g, of which (-1, -1) is the empty value.  Two routines:
//   slsRecordSize   the record's size (0: no record) -- sls_size_kernel, one lane per event
//   slsRecordWord   the four bytes of a record at an aligned position of the output, assembled from whichever pieces cover them
//                   (SlsCursor steps through the items as the positions grow) -- sls_write_kernel, where a lane owns an aligned output
//                   word, and slsWriteRecordHost, which walks the same routine over every word of a record on the host
// Positions inside a record are `padded`: the record's first byte stands at lead = (its output offset & 3), so that padded positions
// which are multiples of four are the output's aligned words.
// Reads: on the device a value is read in aligned dwords that overlap it (the contract for d_data of lc_regex_gpu.h); on the host byte
// by byte, never outside the value.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LC_SLS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_SLS_HD inline
#endif

namespace lcsls {

constexpr uint32_t kMaxItems = 256;         // per list
constexpr uint32_t kMaxKeyBytes = 64u << 10;
constexpr uint32_t kMinLogTime = 1u << 28;  // AddLogTime: below it the varint would be shorter than the five bytes GetLogSize assumes
// a record of this size or more is not written (size 0): positions inside a record are 32-bit
constexpr uint64_t kMaxRecordBytes = 0xFFFFFFF0ull;

struct SlsItem {
    uint32_t prefixAt;   // where in the blob `0x0A varint(klen) key 0x12` begins (4-byte aligned)
    uint32_t prefixLen;  // = S(klen) + 1
    uint32_t source;     // 0: the whole line; g >= 1: capture group g
    uint32_t reserved;
};

// items[0 .. nMatched) for a line the parser matched, items[nMatched .. nMatched + nUnmatched) for every other line
struct SlsPlanView {
    const uint8_t* blob;
    const SlsItem* items;
    uint32_t nMatched, nUnmatched;
};

// one event as the routines see it
struct SlsEvent {
    const uint8_t* line;
    uint32_t lineLen;
    const int32_t* caps;  // int32[2 * ngroups] of this line
    uint32_t firstItem, nItems;
    uint32_t time;
    uint32_t ns;
    bool hasNs;
};

LC_SLS_HD uint32_t varintSize(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }

// tag + varint(v) as little-endian bytes of a 64-bit word (at most six), the bytes behind them zero
LC_SLS_HD uint64_t tagVarint(uint32_t tag, uint32_t v, uint32_t* nbytes) {
    uint64_t w = tag;
    uint32_t at = 1;
    while (v >= 0x80u) {
        w |= uint64_t((v & 0x7Fu) | 0x80u) << (8 * at);
        v >>= 7;
        ++at;
    }
    w |= uint64_t(v) << (8 * at);
    *nbytes = at + 1;
    return w;
}

// the value of an item: [*b, *b + *len) of the line.  A row that does not lie inside the line is cut to it.
LC_SLS_HD void itemValue(const SlsEvent& e, uint32_t source, uint32_t* b, uint32_t* len) {
    if (source == 0) {
        *b = 0;
        *len = e.lineLen;
        return;
    }
    const int32_t cb = e.caps[2 * (source - 1)], ce = e.caps[2 * (source - 1) + 1];
    if (cb < 0 || ce <= cb || uint32_t(cb) >= e.lineLen) {
        *b = 0;
        *len = 0;
        return;
    }
    *b = uint32_t(cb);
    *len = (uint32_t(ce) > e.lineLen ? e.lineLen : uint32_t(ce)) - uint32_t(cb);
}

// which list an event takes (LC_MATCH = 1: the matched one), and whether that makes a record at all
LC_SLS_HD void eventItems(const SlsPlanView& P, uint8_t status, uint32_t* first, uint32_t* count) {
    const bool matched = status == 1;
    *first = matched ? 0 : P.nMatched;
    *count = matched ? P.nMatched : P.nUnmatched;
}

// the bytes of one content on the wire: 1 + varint_size(csz) + csz with csz = S(klen) + S(vlen) = prefixLen + varint_size(vlen) + vlen
LC_SLS_HD uint64_t contentBytes(uint32_t prefixLen, uint32_t vlen, uint32_t* csz) {
    const uint64_t c = uint64_t(prefixLen) + varintSize(vlen) + vlen;
    *csz = uint32_t(c);
    return c >= (1ull << 32) ? kMaxRecordBytes : 1 + varintSize(uint32_t(c)) + c;
}

// GetLogSize over the event's items: the record's bytes, 0 for no record (no items, or too large)
LC_SLS_HD uint64_t slsRecordSize(const SlsPlanView& P, const SlsEvent& e) {
    if (e.nItems == 0) return 0;
    uint64_t logSZ = 6 + (e.hasNs ? 5u : 0u);
    for (uint32_t k = 0; k < e.nItems; ++k) {
        const SlsItem it = P.items[e.firstItem + k];
        uint32_t b, len, csz;
        itemValue(e, it.source, &b, &len);
        logSZ += contentBytes(it.prefixLen, len, &csz);
        if (logSZ >= kMaxRecordBytes) return 0;
    }
    const uint64_t size = 1 + varintSize(uint32_t(logSZ)) + logSZ;
    return size >= kMaxRecordBytes ? 0 : size;
}

// logSZ back from the record's size (size = 1 + varint_size(logSZ) + logSZ grows strictly with logSZ)
LC_SLS_HD uint32_t logSizeOf(uint32_t size) {
    for (uint32_t vs = 1; vs < 5; ++vs)
        if (size >= 1 + vs && varintSize(size - 1 - vs) == vs) return size - 1 - vs;
    return size - 6;
}

// ---- bytes [off, off + 4) of src[0 .. len) as a little-endian word; bytes outside the range read as zero.  off may be -3 .. len - 1.
LC_SLS_HD uint32_t bytes4(const uint8_t* src, uint32_t len, int64_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) + off;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(src), hi = lo + len;
    const uintptr_t base = a & ~uintptr_t(3);
    const uint32_t sh = uint32_t(a & 3u) * 8;
    // only dwords that overlap the value are loaded: they lie inside the 16-byte units around it
    uint32_t w0 = 0, w1 = 0;
    if (base + 4 > lo && base < hi) w0 = *reinterpret_cast<const uint32_t*>(base);
    if (sh && base + 8 > lo && base + 4 < hi) w1 = *reinterpret_cast<const uint32_t*>(base + 4);
    uint32_t w = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
    if (off < 0) w &= 0xFFFFFFFFu << (8 * uint32_t(-off));
    const int64_t over = off + 4 - int64_t(len);
    if (over > 0) w &= 0xFFFFFFFFu >> (8 * uint32_t(over));
    return w;
#else
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) {
        const int64_t at = off + j;
        if (at >= 0 && at < int64_t(len)) w |= uint32_t(src[at]) << (8 * j);
    }
    return w;
#endif
}

// a piece of at most eight computed bytes (v, little-endian, zero behind nbytes) that stands at padded position `at`: its part of word q
LC_SLS_HD uint32_t smallPiece(uint32_t q, uint32_t at, uint32_t nbytes, uint64_t v) {
    if (at >= q + 4 || at + nbytes <= q) return 0;
    return at >= q ? uint32_t(v << (8 * (at - q))) : uint32_t(v >> (8 * (q - at)));
}
// a piece of `len` copied bytes
LC_SLS_HD uint32_t copyPiece(uint32_t q, uint32_t at, uint32_t len, const uint8_t* src) {
    if (len == 0 || at >= q + 4 || uint64_t(at) + len <= q) return 0;
    return bytes4(src, len, int64_t(q) - int64_t(at));
}

// one item of the event laid out at padded position `at`
struct SlsPlaced {
    uint32_t at, total;  // total: the content's bytes on the wire
    uint32_t csz, vb, vlen;
    uint32_t valAt;      // where the value's first byte stands
    SlsItem item;
};
LC_SLS_HD SlsPlaced placeItem(const SlsPlanView& P, const SlsEvent& e, uint32_t k, uint32_t at) {
    SlsPlaced s;
    s.at = at;
    s.item = P.items[e.firstItem + k];
    itemValue(e, s.item.source, &s.vb, &s.vlen);
    s.total = uint32_t(contentBytes(s.item.prefixLen, s.vlen, &s.csz));
    s.valAt = at + s.total - s.vlen;
    return s;
}
LC_SLS_HD uint32_t itemPieces(const SlsPlanView& P, const SlsEvent& e, const SlsPlaced& s, uint32_t q) {
    uint32_t n1, n2;
    const uint64_t head = tagVarint(0x12, s.csz, &n1);
    uint32_t w = smallPiece(q, s.at, n1, head);
    uint32_t at = s.at + n1;
    w |= copyPiece(q, at, s.item.prefixLen, P.blob + s.item.prefixAt);
    at += s.item.prefixLen;
    const uint64_t vl = tagVarint(0, s.vlen, &n2) >> 8;  // (varint(vlen) alone: the 0x12 before it closes the prefix)
    w |= smallPiece(q, at, n2 - 1, vl);
    at += n2 - 1;
    w |= copyPiece(q, at, s.vlen, e.line + s.vb);
    return w;
}

// where a lane stands in a record: the first item that does not end at or before the word it asked for last
struct SlsCursor {
    uint32_t lead, size;   // the record: padded positions [lead, lead + size)
    uint32_t headLen;      // 0x0A varint(logSZ) 0x08 varint5(time)
    uint64_t head0, head1;
    uint32_t head0Len;
    uint32_t k;
    SlsPlaced cur;
};
LC_SLS_HD SlsCursor slsCursorBegin(const SlsPlanView& P, const SlsEvent& e, uint32_t lead, uint32_t size) {
    SlsCursor c;
    c.lead = lead;
    c.size = size;
    c.head0 = tagVarint(0x0A, logSizeOf(size), &c.head0Len);
    uint32_t n;
    c.head1 = tagVarint(0x08, e.time < kMinLogTime ? kMinLogTime : e.time, &n);  // (always six bytes)
    c.headLen = c.head0Len + 6;
    c.k = 0;
    c.cur = placeItem(P, e, 0, lead + c.headLen);
    return c;
}
// the word at padded position q (a multiple of four; q + 4 > lead, q < lead + size; q must not go down between calls).  Bytes outside
// the record are zero.
LC_SLS_HD uint32_t slsRecordWord(const SlsPlanView& P, const SlsEvent& e, SlsCursor& c, uint32_t q) {
    while (c.k + 1 < e.nItems && c.cur.at + c.cur.total <= q) {
        ++c.k;
        c.cur = placeItem(P, e, c.k, c.cur.at + c.cur.total);
    }
    // most words of a record lie inside one value: four of its bytes and nothing else
    if (q >= c.cur.valAt && q + 4 <= c.cur.valAt + c.cur.vlen) return bytes4(e.line + c.cur.vb, c.cur.vlen, int64_t(q - c.cur.valAt));
    uint32_t w = smallPiece(q, c.lead, c.head0Len, c.head0) | smallPiece(q, c.lead + c.head0Len, 6, c.head1);
    w |= itemPieces(P, e, c.cur, q);
    // a content is six bytes or more: a word touches at most one more after the first
    uint32_t next = c.cur.at + c.cur.total;
    for (uint32_t k = c.k + 1; k < e.nItems && next < q + 4; ++k) {
        const SlsPlaced s = placeItem(P, e, k, next);
        w |= itemPieces(P, e, s, q);
        next += s.total;
    }
    if (e.hasNs) w |= smallPiece(q, c.lead + c.size - 5, 5, 0x25u | (uint64_t(e.ns) << 8));
    return w;
}

// The record of one event at out[at .. at + size), size = slsRecordSize(...) > 0, through slsRecordWord as the device walks it: every
// aligned word of the output the record overlaps, of which the first and the last may be partial.  Touches no byte outside the record.
inline void slsWriteRecordHost(const SlsPlanView& P, const SlsEvent& e, uint8_t* out, uint64_t at, uint32_t size) {
    const uint32_t lead = uint32_t(at & 3u);
    SlsCursor c = slsCursorBegin(P, e, lead, size);
    for (uint32_t q = 0; q < lead + size; q += 4) {
        const uint32_t w = slsRecordWord(P, e, c, q);
        for (uint32_t j = 0; j < 4; ++j)
            if (q + j >= lead && q + j < lead + size) out[at - lead + q + j] = uint8_t(w >> (8 * j));
    }
}

}  // namespace lcsls
