// delim_vm.hpp -- the per-line routine of the delimiter parser, ONE function for the host and the device.
//
// delimSplitLine() does for one line what ProcessorParseDelimiterNative::ProcessEvent does before it touches the event
// (core/plugin/processor/ProcessorParseDelimiterNative.cpp:220-282): the trim (:226-242), then either the quote-aware four-state
// machine of core/parser/DelimiterModeFsmParser.cpp (the StringView overloads :49-81, :134-154, :172-186, :201-223, :260-294) or
// SplitString (:366-409).  It never touches memory itself: the bytes come from a SOURCE (template parameter) that hands out 16-byte
// quads in "tile coordinates" -- position 0 is the 16-byte boundary at or below the line's first byte, the line occupies
// [head, head + len) -- because that is how the kernel (delim_kernel.hpp) stages lines: 64-byte rows of aligned 16-byte loads.
//
//   struct Source {
//       uint32_t head() const;                          // 0..15
//       void tailQuad(uint32_t p16, uint32_t q[4]);     // the quad at tile position p16 (multiple of 16), straight from memory
//       uint32_t stageCount(uint32_t end);              // 64-byte stages to walk for a line that ends (trimmed) at tile position end;
//                                                       //   the device answers for the whole WAVEFRONT (the stage loop is uniform)
//       void stage(uint32_t s);                         // make stage s current (the device: cooperative load into the LDS tile)
//       void rowQuad(uint32_t k, uint32_t q[4]);        // quad k (0..3) of the current stage of THIS line
//   };
//
// The host source (HostLineSource below) answers from a byte pointer and returns junk for every byte outside the line, so the CPU suite
// (tests/native/delimiter_double.cpp) proves that no byte outside [head, head + len) is ever interpreted.
//
// Output: status (LC_DELIM_OK / LC_DELIM_FAIL / LC_DELIM_BLANK: nothing behind the trim), the TRUE column count, and the first min(count, W) columns as (begin, end) relative to
// the line's first byte.  On the quote path a column's span excludes its enclosing quotes; a column that holds doubled quotes has
// bit 31 of `begin` set (kDelimDoubledFlag): its value is not a view of the line, the host un-doubles it (AddFieldWithUnQuote :83-113).
// A failed line reports zero columns (the reference clears them, :283-291).
#pragma once

#include <stdint.h>

#include "../../include/lc_delimiter.h"

#if defined(__HIPCC__)
#define LC_DELIM_HD __host__ __device__ __forceinline__
#else
#define LC_DELIM_HD inline
#endif

constexpr uint32_t kDelimDoubledFlag = 0x80000000u;
constexpr uint32_t kDelimStageBytes = 64;

// what lc_delim_create fixes; passed to the kernel by value
struct DelimConfig {
    uint32_t sepWord;   // plain path: the separator's bytes as the low bytes of a rolling window (last byte lowest)
    uint32_t sepMask;   // plain path: the window bits that take part
    uint32_t sepLen;    // 1..4
    uint32_t nKeys;     // plain path, stopAtKeys: the walk ends once this many columns exist and a separator follows
    uint8_t sep0;       // quote path: the separator byte
    uint8_t quote;      // quote path: the quote byte
    uint8_t useQuote;   // separator of one byte and Quote != Separator (:251)
    uint8_t stopAtKeys; // OverflowedFieldsTreatment is keep or discard (:398)
};

// ProcessorParseDelimiterNative.cpp:56-70 (the separator), :109 (the parser's two bytes), :251 (which path), :398 (the early stop).
// false: no separator of 1..4 bytes, or no such mode
inline bool delimMakeConfig(const uint8_t* separator, uint32_t sepLen, uint8_t quote, int mode, uint32_t nKeys, DelimConfig* out) {
    if (!separator || sepLen < 1 || sepLen > 4 || mode < LC_DELIM_EXTEND || mode > LC_DELIM_DISCARD) return false;
    DelimConfig c{};
    for (uint32_t i = 0; i < sepLen; ++i) c.sepWord = (c.sepWord << 8) | separator[i];
    c.sepMask = sepLen == 4 ? 0xFFFFFFFFu : ((1u << (8 * sepLen)) - 1u);
    c.sepLen = sepLen;
    c.nKeys = nKeys;
    c.sep0 = separator[0];
    c.quote = quote;
    c.useQuote = (sepLen == 1 && quote != separator[0]) ? 1 : 0;
    c.stopAtKeys = mode != LC_DELIM_EXTEND ? 1 : 0;
    *out = c;
    return true;
}

struct alignas(8) DelimSpan {
    int32_t begin, end;
};

enum : uint32_t { kDelimInitial = 0, kDelimQuote = 1, kDelimData = 2, kDelimDoubleQuote = 3 };

struct DelimWalk {
    uint32_t fs = 0, fe = 0;  // quote path: fieldStart / fieldEnd; plain path: fs = start of the current column
    uint32_t state = kDelimInitial;
    uint32_t dq = 0;          // doubleQuoteNum
    uint32_t ncols = 0;       // TRUE count
    uint32_t win = 0;         // plain path: the last four bytes
    bool failed = false, done = false;
};

LC_DELIM_HD void delimEmit(DelimWalk& w, uint32_t b, uint32_t e, bool doubled, uint32_t W, DelimSpan* row) {
    if (w.ncols < W) row[w.ncols] = DelimSpan{int32_t(b | (doubled ? kDelimDoubledFlag : 0u)), int32_t(e)};
    ++w.ncols;
}

// one byte of the quote path; i is not needed: the reference's machine counts its own way through the line
LC_DELIM_HD void delimStepQuote(const DelimConfig& c, DelimWalk& w, uint32_t ch, uint32_t W, DelimSpan* row) {
    if (ch == c.sep0) {  // HandleSeparator :49-81
        if (w.state == kDelimQuote) {
            ++w.fe;
        } else if (w.state == kDelimDoubleQuote) {
            w.state = kDelimInitial;
            --w.dq;
            delimEmit(w, w.fs, w.fe, w.dq != 0, W, row);
            w.dq = 0;
            w.fe += 2;  // (the closing quote and the separator)
            w.fs = w.fe;
        } else {  // INITIAL, DATA
            w.state = kDelimInitial;
            delimEmit(w, w.fs, w.fe, w.dq != 0, W, row);
            w.dq = 0;
            w.fs = ++w.fe;
        }
    } else if (ch == c.quote) {  // HandleQuote :134-154
        if (w.state == kDelimInitial) {
            w.state = kDelimQuote;
            ++w.fs;
        } else if (w.state == kDelimQuote) {
            w.state = kDelimDoubleQuote;
            ++w.dq;
            ++w.fe;
        } else if (w.state == kDelimDoubleQuote) {
            w.state = kDelimQuote;
            ++w.fe;
        } else {
            w.failed = true;  // a quote in DATA
        }
    } else {  // HandleData :172-186
        if (w.state == kDelimDoubleQuote) {
            w.failed = true;  // data after a closing quote
        } else {
            if (w.state == kDelimInitial) w.state = kDelimData;
            ++w.fe;
        }
    }
}

// one byte of SplitString (:377-403) at line position i; end = the trimmed end of the line
LC_DELIM_HD void delimStepPlain(const DelimConfig& c, DelimWalk& w, uint32_t ch, uint32_t i, uint32_t end, uint32_t W, DelimSpan* row) {
    w.win = (w.win << 8) | ch;
    if (i + 1 - w.fs < c.sepLen || (w.win & c.sepMask) != c.sepWord) return;
    const uint32_t at = i + 1 - c.sepLen;  // std::search from the column's start: the leftmost separator that begins at or behind it
    delimEmit(w, w.fs, at, false, W, row);
    w.fs = i + 1;
    if (c.stopAtKeys && w.ncols >= c.nKeys) {  // :398-402: the remainder column BEGINS AT the separator
        delimEmit(w, at, end, false, W, row);
        w.done = true;
    }
}

// QUOTE: the quote path (c.useQuote); a template parameter so that the per-byte code holds one machine, not both
template <bool QUOTE, class Source>
LC_DELIM_HD void delimSplitLine(const DelimConfig& c, Source& src, uint32_t len, uint32_t W, DelimSpan* row, uint8_t* statusOut,
                                uint32_t* ncolsOut) {
    const uint32_t head = src.head();
    // ---- :226-231: trailing ' ' and '\r'.  The quads at the line's end, walked backwards (almost always one)
    uint32_t end = head + len;  // tile position
    {
        bool more = len != 0;
        while (more) {
            const uint32_t p16 = (end - 1) & ~15u;
            uint32_t q[4];
            src.tailQuad(p16, q);
            const uint32_t lo = p16 > head ? p16 : head;
            while (end > lo) {
                const uint32_t j = end - 1 - p16;
                const uint32_t ch = (q[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
                if (ch != ' ' && ch != '\r') {
                    more = false;
                    break;
                }
                --end;
            }
            if (end <= head) more = false;
        }
    }
    // ---- the walk: 64-byte stages, the same number for every line of a wavefront
    DelimWalk w;
    bool leading = true;      // :232-238: leading ' '
    uint32_t begin = head;    // tile position of the first byte behind them
    const uint32_t lineEnd = end - head;
    const uint32_t stages = src.stageCount(end > head ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kDelimStageBytes;
        if (base >= end || w.failed || w.done) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kDelimStageBytes / 16; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t p = qbase + j;
                if (p < begin || p >= end || w.failed || w.done) continue;
                const uint32_t ch = (q[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
                if (leading) {
                    if (ch == ' ') {
                        begin = p + 1;
                        continue;
                    }
                    leading = false;
                    w.fs = w.fe = p - head;
                }
                if (QUOTE) delimStepQuote(c, w, ch, W, row);
                else delimStepPlain(c, w, ch, p - head, lineEnd, W, row);
            }
        }
    }
    // ---- the line's end.  :239-242: nothing left behind the trim is a failure
    const bool blank = len == 0 || begin >= end || leading;
    if (blank) w.failed = true;
    if (!w.failed && !w.done) {
        if (QUOTE) {  // HandleEOF :201-223
            if (w.state == kDelimDoubleQuote) --w.dq;
            if (w.state == kDelimQuote) w.failed = true;  // the line ends inside a quote
            else delimEmit(w, w.fs, w.fe, w.dq != 0, W, row);
        } else {
            delimEmit(w, w.fs, lineEnd, false, W, row);  // :383-396, :404-407: what is left is the last column (it may be empty)
        }
    }
    *statusOut = blank ? LC_DELIM_BLANK : w.failed ? LC_DELIM_FAIL : LC_DELIM_OK;
    *ncolsOut = w.failed ? 0u : w.ncols;
}

// the host's source: a byte pointer; every byte outside the line reads as junk that is neither blank nor likely a separator
struct HostLineSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    HostLineSource(const uint8_t* l, uint32_t n, uint32_t head) : line(l), len(n), headBytes(head & 15u) {}
    uint32_t head() const { return headBytes; }
    void quadAt(uint32_t p16, uint32_t q[4]) const {
        for (int k = 0; k < 4; ++k) q[k] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = p16 + j;
            const uint32_t b = (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : (j & 1 ? 0x20u : 0x22u);  // junk: ' ' and '"'
            q[j >> 2] |= b << ((j & 3) * 8);
        }
    }
    void tailQuad(uint32_t p16, uint32_t q[4]) const { quadAt(p16, q); }
    uint32_t stageCount(uint32_t end) const { return (end + kDelimStageBytes - 1) / kDelimStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const { quadAt(stageNow * kDelimStageBytes + k * 16, q); }
};
