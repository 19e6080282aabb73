// apsara_vm.hpp -- the per-line routine of the Apsara parser, ONE function for the host and the device.
//
// apsaraParseLine() does for one line what ProcessorParseApsaraNative::ProcessEvent does before it touches the event
// (core/plugin/processor/ProcessorParseApsaraNative.cpp): the time without the per-group cache (ApsaraEasyReadLogTimeParser :251-323),
// the base-field scan and its classification (FindBaseFields / ParseApsaraBaseFields :342-463) and the key:value walk (:202-224).  The
// bytes come from a SOURCE in tile coordinates, as in delim_vm.hpp: position 0 is the 16-byte boundary at or below the line's first
// byte, the line occupies [head, head + len), and is walked ONCE in 64-byte stages.
//
//   struct Source {
//       uint32_t head() const;                 // 0..15
//       uint32_t stageCount(uint32_t end);     // 64-byte stages for a line that ends at tile position end (the device: of the wavefront)
//       void stage(uint32_t s);                // make stage s current
//       void rowQuad(uint32_t k, uint32_t q[4]);   // quad k (0..3) of the current stage of THIS line
//       uint32_t timeByte(uint32_t p) const;   // the byte at tile position p (head < p < head + len) WHILE STAGE 0 IS CURRENT: the
//   };                                         //   time text lies there (the device: an LDS read; behind byte 63 a re-read from memory)
//
// The time reuses strptime_vm.hpp: tsConvNum (conv_num), tsConvNanos ("%f"), tsConvEpoch ("%s" and its tail rule), tsCivilSeconds.
// The two formats are fixed, so they are straight-line code here and no program is staged.  The view the reference hands to Strptime
// ends at the first ']' behind byte 0; neither format can step over a ']', so the routine reads the line itself and asks at the end
// whether a ']' was met at all (a line without one fails, :279-283).
//
// The scan and the pair walk are byte-at-a-time machines.  FindBaseFields looks one and two bytes ahead of a ']' (:348, :355): the
// machine decides one and two bytes LATER instead (states kScanBracket, kScanTab).  The pair walk starts behind the LAST field the scan
// closes, which is known only when the scan stops: the walk runs from byte 1 on and starts over (count 0) at every field that closes --
// at most ten times, and only the pairs of the last start are left in the row.
#pragma once

#include <stdint.h>

#include "../../include/lc_apsara.h"
#include "strptime_vm.hpp"

constexpr uint32_t kApsaraStageBytes = 64;
constexpr uint32_t kApsaraMaxBaseFields = 10;  // MAX_BASE_FIELD_NUM

struct ApsaraPair {
    int32_t keyBegin, colon, end;  // key = [keyBegin, colon), value = (colon, end)
};
struct ApsaraSpan {
    int32_t begin, end;
};
struct ApsaraLine {
    uint8_t status;
    int64_t secs;
    uint32_t nanos;
    ApsaraSpan base[4];
    uint32_t npairs;  // TRUE count
};

// the time text behind '[': at(i) = line byte 1 + i
template <class Source>
struct ApsaraTimeView {
    const Source& src;
    uint32_t first;  // tile position of line byte 1
    LC_TS_HD uint32_t at(uint32_t i) const { return src.timeByte(first + i); }
};

// ApsaraEasyReadLogTimeParser's two Strptime calls over the n bytes behind '[' (:259-276 and :301-315).  No cache, no zone.
// status: LC_APSARA_TIME_OK still lacks the "a ']' exists" half
template <class View>
LC_TS_HD void apsaraTime(const View& t, uint32_t n, uint8_t& status, int64_t& secs, uint32_t& nanos) {
    status = 0;
    secs = 0;
    nanos = 0;
    int32_t fracLen = 0;
    if (n == 0) return;
    if (t.at(0) == '1') {  // :259
        status = LC_APSARA_EPOCH;
        uint32_t pos = 0;
        int64_t s = 0;
        if (tsConvEpoch(t, n, s, nanos, fracLen, pos) && pos < n && t.at(pos) == ']') {  // :269-273
            status |= LC_APSARA_TIME_OK;
            secs = s;
        }
        return;
    }
    // "%Y-%m-%d %H:%M:%S" (:301)
    uint32_t pos = 0;
    int32_t year = 1900, mon1 = 1, mday = 0, hour = 0, min = 0, sec = 0;
    bool ok = tsConvNum(t, n, pos, 0, 9999, year);
    ok = ok && pos < n && t.at(pos++) == '-' && tsConvNum(t, n, pos, 1, 12, mon1);
    ok = ok && pos < n && t.at(pos++) == '-' && tsConvNum(t, n, pos, 1, 31, mday);
    if (ok)
        while (pos < n && tsIsSpace(t.at(pos))) ++pos;
    ok = ok && tsConvNum(t, n, pos, 0, 23, hour);
    ok = ok && pos < n && t.at(pos++) == ':' && tsConvNum(t, n, pos, 0, 59, min);
    ok = ok && pos < n && t.at(pos++) == ':' && tsConvNum(t, n, pos, 0, 61, sec);
    if (!ok) return;
    status = uint8_t(LC_APSARA_TIME_OK | (pos == 19 ? LC_APSARA_CANON19 : 0u));
    secs = tsCivilSeconds(year, uint32_t(mon1 - 1), mday, int64_t(hour) * 3600 + int64_t(min) * 60 + int64_t(sec));
    // :308-315: "%f" one byte further on, unless the view ends here (its last byte is the ']'; a NUL ends the reference's C string)
    if (pos < n) {
        const uint32_t c = t.at(pos);
        if (c != ']' && c != 0u) {
            uint32_t q = pos + 1;
            (void)tsConvNanos(t, n, q, nanos, fracLen);
        }
    }
}

enum : uint32_t { kScanOpen = 0, kScanBracket = 1, kScanTab = 2, kScanStopped = 3 };
constexpr uint32_t kApsaraNone = 0xFFFFFFFFu;
// flag bits of the bytes of a field
enum : uint32_t { kNotUpper = 1, kNotDigit = 2, kSlashDot = 4 };

struct ApsaraWalk {
    // the scan
    uint32_t scan = kScanOpen, nFields = 0, found = 0;
    uint32_t begin = 0;                  // beginIndexArray[nFields]: 0 until a '[' moves it
    uint32_t flags = 0, colon = kApsaraNone;           // of the bytes behind the last '['
    uint32_t pendFlags = 0;              // ... as they were in front of the ']' that may close the field
    uint32_t zeroSlashDot = 0, zeroColon = kApsaraNone;  // of the bytes from the line's first byte on (a field whose begin stayed 0)
    bool fromZero = true, sawBracket = false;
    // the pair walk
    uint32_t npairs = 0, pairBegin = 0, pairColon = kApsaraNone;
};

// a field closes at the ']' at line position e (:348-351), then ParseApsaraBaseFields' loop body for it (:443-461)
LC_TS_HD void apsaraCloseField(ApsaraWalk& w, uint32_t e, ApsaraSpan* base) {
    const uint32_t k = w.nFields++;
    if (k >= 1 && w.found != 7u) {
        // a field that begins at byte 0 holds the line's '[' (a line without it has no time and is never stitched)
        const uint32_t b = w.fromZero ? 0u : w.begin;
        const uint32_t f = w.fromZero ? (kNotUpper | kNotDigit | w.zeroSlashDot) : w.pendFlags;
        const uint32_t c = w.fromZero ? w.zeroColon : w.colon;
        if (!(w.found & 1u) && !(f & kNotUpper)) {
            w.found |= 1u;
            base[LC_APSARA_LEVEL] = ApsaraSpan{int32_t(b), int32_t(e)};
        } else if (!(w.found & 2u) && !(f & kNotDigit)) {
            w.found |= 2u;
            base[LC_APSARA_THREAD] = ApsaraSpan{int32_t(b), int32_t(e)};
        } else if (!(w.found & 4u) && (f & kSlashDot)) {
            w.found |= 4u;
            base[LC_APSARA_FILE] = ApsaraSpan{int32_t(b), int32_t(c != kApsaraNone ? c : e)};
            if (c != kApsaraNone) base[LC_APSARA_LINE] = ApsaraSpan{int32_t(c + 1), int32_t(e)};
        }
    }
    w.begin = 0;
    w.fromZero = true;
    // the pair walk starts behind this ']' (:205-208), with beg_index = 0
    w.npairs = 0;
    w.pairBegin = 0;
    w.pairColon = kApsaraNone;
}

LC_TS_HD void apsaraEmitPair(ApsaraWalk& w, uint32_t end, uint32_t W, ApsaraPair* row) {
    if (w.npairs < W) row[w.npairs] = ApsaraPair{int32_t(w.pairBegin), int32_t(w.pairColon), int32_t(end)};
    ++w.npairs;
}

// line byte i
LC_TS_HD void apsaraStep(ApsaraWalk& w, uint32_t ch, uint32_t i, uint32_t W, ApsaraSpan* base, ApsaraPair* row) {
    // ---- what the ']' one or two bytes back was waiting for
    if (w.scan == kScanBracket) {
        if (ch == '\t' || ch == '\n') {
            apsaraCloseField(w, i - 1, base);
            w.scan = w.nFields >= kApsaraMaxBaseFields ? kScanStopped : (ch == '\t' ? kScanTab : kScanOpen);  // :352-357
        } else {
            w.scan = kScanOpen;
        }
    } else if (w.scan == kScanTab) {
        w.scan = ch == '[' ? kScanOpen : kScanStopped;  // :355
    }
    // ---- FindBaseFields' own look at byte i
    if (ch == '/' || ch == '.') w.zeroSlashDot = kSlashDot;
    if (ch == ':' && w.zeroColon == kApsaraNone) w.zeroColon = i;
    if (w.scan == kScanOpen) {
        if (ch == '[') {
            w.begin = i + 1;
            w.fromZero = false;
            w.flags = 0;
            w.colon = kApsaraNone;
        } else {
            if (ch == ']') {
                w.scan = kScanBracket;
                w.sawBracket = true;
                w.pendFlags = w.flags;
            }
            if (ch - 'A' >= 26u) w.flags |= kNotUpper;
            if (ch - '0' >= 10u) w.flags |= kNotDigit;
            if (ch == '/' || ch == '.') w.flags |= kSlashDot;
            if (ch == ':' && w.colon == kApsaraNone) w.colon = i;
        }
    }
    // ---- the pair walk (:208-223); byte 0 is never its
    if (i >= 1) {
        if (ch == '\t') {
            if (w.pairColon != kApsaraNone) {
                apsaraEmitPair(w, i, W, row);
                w.pairColon = kApsaraNone;
            }
            w.pairBegin = i + 1;
        } else if (ch == ':' && w.pairColon == kApsaraNone) {
            w.pairColon = i;
        }
    }
}

// row: room for W pairs.  Nothing behind the line's end is interpreted.
template <class Source>
LC_TS_HD void apsaraParseLine(Source& src, uint32_t len, uint32_t W, ApsaraPair* row, ApsaraLine& out) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;
    ApsaraWalk w;
    for (int k = 0; k < 4; ++k) out.base[k] = ApsaraSpan{-1, -1};
    out.status = 0;
    out.secs = 0;
    out.nanos = 0;
    bool opens = false;
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kApsaraStageBytes;
        if (base >= end) continue;
        if (s == 0 && len >= 2) {
            const ApsaraTimeView<Source> view{src, head + 1};
            apsaraTime(view, len - 1, out.status, out.secs, out.nanos);
        }
#pragma unroll 1
        for (uint32_t k = 0; k < kApsaraStageBytes / 16; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t p = qbase + j;
                if (p < head || p >= end) continue;
                const uint32_t ch = (q[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
                if (p == head) opens = ch == '[';  // :255
                apsaraStep(w, ch, p - head, W, out.base, row);
            }
        }
    }
    // ---- the line's end: a ']' as the last byte closes its field (:348, i + 1 == size); what is left of a pair is flushed (:209)
    if (w.scan == kScanBracket) apsaraCloseField(w, len - 1, out.base);
    if (w.pairColon != kApsaraNone) apsaraEmitPair(w, len, W, row);
    if (!(opens && w.sawBracket)) out.status &= uint8_t(~(LC_APSARA_TIME_OK | LC_APSARA_CANON19));
    out.npairs = w.npairs;
}

// the host's source: a byte pointer; every byte outside the line reads as junk the machines would react to (']', TAB, ':')
struct ApsaraHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    ApsaraHostSource(const uint8_t* l, uint32_t n, uint32_t head) : line(l), len(n), headBytes(head & 15u) {}
    uint32_t head() const { return headBytes; }
    uint32_t stageCount(uint32_t end) const { return (end + kApsaraStageBytes - 1) / kApsaraStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kApsaraStageBytes + k * 16;
        for (int d = 0; d < 4; ++d) q[d] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = p16 + j;
            const uint32_t b = (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : (j % 3 == 0 ? uint32_t(']') : j % 3 == 1 ? uint32_t('\t') : uint32_t(':'));
            q[j >> 2] |= b << ((j & 3) * 8);
        }
    }
    uint32_t timeByte(uint32_t p) const { return line[p - headBytes]; }
};

// one line on the host, through the routine (the CPU double, the processor's replay, the tools)
inline void apsaraParseHost(const uint8_t* line, uint32_t len, uint32_t W, ApsaraPair* row, ApsaraLine& out, uint32_t head = 0) {
    ApsaraHostSource src(line, len, head);
    apsaraParseLine(src, len, W, row, out);
}
