// csv_vm.hpp -- the per-value routine of the CSV decoder, ONE function for the host and the device.
//
// csvReadRecord() gives for one value what r.Read() returns for csv.NewReader(strings.NewReader(value)) of Go 1.23's encoding/csv with
// Comma = the separator, TrimLeadingSpace as configured, LazyQuotes = false, Comment = 0, FieldsPerRecord = 0: the FIRST record as spans,
// or an error (include/csv/lc_csv.h).  The Go reads line by line and rewrites each line's end; this routine makes ONE forward pass over
// the value's own bytes and states the line rules on them:
//   * kCsvLine (before the record): a `\n`, a `\r\n`, and a `\r` that is the value's last byte are empty lines and are skipped -- before
//     any trimming.  Nothing left: LC_CSV_EOF.
//   * kCsvField (a field begins): with TrimLeadingSpace the unicode.IsSpace runes are passed, byte by byte, up to and INCLUDING the line's
//     own `\n` (then the field is empty and the record ends: the trim never enters the next line).  A `"` opens a quoted field.
//   * kCsvUnquoted: the next separator in the line ends the field, the line's `\n` ends the field and the record -- without the one `\r`
//     before it; so does the value's end, without one `\r`.  A `"` met first is LC_CSV_BARE_QUOTE.
//   * kCsvQuoted: only `"` matters (and `\r`, which marks the field as one to fold: `\r\n` -> `\n`).  The value's end is LC_CSV_QUOTE.
//   * kCsvAfterQuote (the byte behind a `"` inside quotes): `"` is a literal quote (fold), the separator ends the field, `\n`, `\r\n`,
//     a `\r` as the value's last byte and the value's end end the field and the record, anything else is LC_CSV_QUOTE.
// The first three of these look at every byte; the two field phases jump (the quad skip, as kv_vm.hpp): per 16-byte quad one 16-bit mask
// for the separator's first byte, `"`, `\n` and `\r`, the phase ORs the ones it cares about and goes to the first set bit.  A separator
// of 2 to 4 bytes is confirmed there; its bytes are a word the caller holds (kernel argument), no memory is read for them.
//
// The routine never touches memory itself: the bytes come from a SOURCE (the contract of kv_vm.hpp): head(), stageCount(end), stage(s),
// rowQuad(k, q), byteAt(p) in tile coordinates -- and it asks for no byte outside the value.
#pragma once

#include <stdint.h>

#include "../../include/csv/lc_csv.h"

#if defined(__HIPCC__)
#define LC_CSV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_CSV_HD inline
#endif

constexpr uint32_t kCsvStageBytes = 64;

// what lc_csv_create fixes: the separator's UTF-8 bytes, first byte lowest, and their count
struct CsvConfig {
    uint32_t sepWord = ',';
    uint32_t sepLen = 1;  // 1..4
    uint32_t trim = 0;
    uint32_t invalidDelim = 0;  // `"`, \r, \n, U+0000, U+FFFD: every Read fails
};

enum : uint32_t { kCsvLine = 0, kCsvField = 1, kCsvUnquoted = 2, kCsvQuoted = 3, kCsvAfterQuote = 4, kCsvDone = 5 };

struct CsvWalk {
    uint32_t cur = 0;  // the next position to look at
    uint32_t fb = 0;   // the current field's first byte (behind the quote for a quoted one)
    uint32_t fold = 0;
    uint32_t phase = kCsvLine;
    uint32_t nfields = 0;
    uint32_t status = LC_CSV_OK;
};

// one bit per byte of the quad q (bit j = byte j) that equals the byte spread over b4 (exact: no carry crosses a byte)
LC_CSV_HD uint32_t csvEqNibble(uint32_t x, uint32_t b4) {
    const uint32_t y = x ^ b4;
    const uint32_t u = (~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) >> 7;
    return (u | (u >> 7) | (u >> 14) | (u >> 21)) & 0xFu;
}
LC_CSV_HD uint32_t csvEqQuad(const uint32_t q[4], uint32_t b4) {
    return csvEqNibble(q[0], b4) | (csvEqNibble(q[1], b4) << 4) | (csvEqNibble(q[2], b4) << 8) | (csvEqNibble(q[3], b4) << 12);
}
// the bits lo .. hi - 1 of a quad's mask (lo, hi: any integers; clamped to 0..16)
LC_CSV_HD uint32_t csvBitRange(int32_t lo, int32_t hi) {
    const uint32_t below = lo <= 0 ? 0xFFFFu : lo >= 16 ? 0u : (0xFFFFu << lo) & 0xFFFFu;
    const uint32_t above = hi >= 16 ? 0xFFFFu : hi <= 0 ? 0u : (1u << hi) - 1u;
    return below & above;
}

// the separator at value position pos, whose byte there is c
template <class Source>
LC_CSV_HD bool csvIsSep(const Source& src, uint32_t head, uint32_t len, uint32_t sepWord, uint32_t sepLen, uint32_t pos, uint32_t c) {
    if (c != (sepWord & 0xFFu) || pos + sepLen > len) return false;
    for (uint32_t j = 1; j < sepLen; ++j)
        if (src.byteAt(head + pos + j) != ((sepWord >> (8 * j)) & 0xFFu)) return false;
    return true;
}

// bytes of the unicode.IsSpace rune at pos (c: its first byte), 0 for anything else -- malformed and truncated UTF-8 included
template <class Source>
LC_CSV_HD uint32_t csvSpaceRune(const Source& src, uint32_t head, uint32_t len, uint32_t pos, uint32_t c) {
    if (c == ' ' || (c >= 9 && c <= 13)) return 1;
    if (c == 0xC2u && pos + 2 <= len) {  // U+0085, U+00A0
        const uint32_t d = src.byteAt(head + pos + 1);
        return (d == 0x85u || d == 0xA0u) ? 2u : 0u;
    }
    if ((c == 0xE1u || c == 0xE2u || c == 0xE3u) && pos + 3 <= len) {
        const uint32_t d = src.byteAt(head + pos + 1), e = src.byteAt(head + pos + 2);
        const bool ogham = c == 0xE1u && d == 0x9Au && e == 0x80u;                                                              // U+1680
        const bool general = c == 0xE2u && d == 0x80u && ((e >= 0x80u && e <= 0x8Au) || e == 0xA8u || e == 0xA9u || e == 0xAFu);  // U+2000..200A, 2028, 2029, 202F
        const bool math = c == 0xE2u && d == 0x81u && e == 0x9Fu;                                                               // U+205F
        const bool ideographic = c == 0xE3u && d == 0x80u && e == 0x80u;                                                        // U+3000
        return (ogham || general || math || ideographic) ? 3u : 0u;
    }
    return 0;
}

template <class Sink>
LC_CSV_HD void csvEmit(Sink& sink, CsvWalk& w, uint32_t b, uint32_t e, uint32_t fold) {
    sink.field(w.nfields, int32_t(b | (fold ? LC_CSV_FOLD : 0u)), int32_t(e));
    ++w.nfields;
}

// the byte at value position pos == w.cur (kCsvLine, kCsvField, kCsvAfterQuote) or the first byte at or behind w.cur the phase asked for
template <bool Trim, class Source, class Sink>
LC_CSV_HD void csvEvent(const Source& src, Sink& sink, CsvWalk& w, uint32_t head, uint32_t len, uint32_t sepWord, uint32_t sepLen, uint32_t pos) {
    const uint32_t c = src.byteAt(head + pos);
    w.cur = pos + 1;
    if (w.phase == kCsvLine) {  // empty lines, before any trimming
        if (c == '\n') return;
        if (c == '\r') {
            if (pos + 1 == len) return;  // the last line loses its `\r` and is empty: io.EOF at the value's end
            if (src.byteAt(head + pos + 1) == '\n') {
                w.cur = pos + 2;
                return;
            }
        }
        w.phase = kCsvField;
    }
    if (w.phase == kCsvField) {
        if (Trim) {
            if (c == '\n') {  // the trim ate the line's end: an empty field, and the record ends
                csvEmit(sink, w, pos, pos, 0);
                w.phase = kCsvDone;
                return;
            }
            const uint32_t sp = csvSpaceRune(src, head, len, pos, c);
            if (sp) {
                w.cur = pos + sp;
                return;
            }
        }
        w.fold = 0;
        if (c == '"') {
            w.fb = pos + 1;
            w.phase = kCsvQuoted;
            return;
        }
        w.fb = pos;
        w.phase = kCsvUnquoted;
    }
    if (w.phase == kCsvUnquoted) {
        if (c == '"') {
            w.status = LC_CSV_BARE_QUOTE;
            w.phase = kCsvDone;
        } else if (c == '\n') {
            const uint32_t e = (pos > w.fb && src.byteAt(head + pos - 1) == '\r') ? pos - 1 : pos;
            csvEmit(sink, w, w.fb, e, 0);
            w.phase = kCsvDone;
        } else if (csvIsSep(src, head, len, sepWord, sepLen, pos, c)) {
            csvEmit(sink, w, w.fb, pos, 0);
            w.cur = pos + sepLen;
            w.phase = kCsvField;
        }
        return;
    }
    if (w.phase == kCsvQuoted) {
        if (c == '"') w.phase = kCsvAfterQuote;
        else w.fold = 1;  // a `\r`: the host looks whether a `\n` follows it
        return;
    }
    // kCsvAfterQuote: pos - 1 is a `"` inside quotes
    if (c == '"') {
        w.fold = 1;
        w.phase = kCsvQuoted;
    } else if (csvIsSep(src, head, len, sepWord, sepLen, pos, c)) {
        csvEmit(sink, w, w.fb, pos - 1, w.fold);
        w.cur = pos + sepLen;
        w.phase = kCsvField;
    } else if (c == '\n' || (c == '\r' && (pos + 1 == len || src.byteAt(head + pos + 1) == '\n'))) {
        csvEmit(sink, w, w.fb, pos - 1, w.fold);
        w.phase = kCsvDone;
    } else {
        w.status = LC_CSV_QUOTE;
        w.phase = kCsvDone;
    }
}

// Sink: void field(uint32_t k, int32_t begin, int32_t end) -- row k of the value (the sink drops k >= W)
template <bool Trim, class Source, class Sink>
LC_CSV_HD void csvReadRecord(Source& src, Sink& sink, uint32_t len, uint32_t sepWord, uint32_t sepLen, uint8_t* statusOut, uint32_t* countOut) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;  // tile position
    const uint32_t s4 = (sepWord & 0xFFu) * 0x01010101u;
    CsvWalk w;
    const uint32_t stages = src.stageCount(len != 0 ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kCsvStageBytes;
        if (w.phase == kCsvDone || base >= end || base + kCsvStageBytes <= head + w.cur) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kCsvStageBytes / 16; ++k) {
            const uint32_t qbase = base + k * 16;
            if (w.phase == kCsvDone || qbase >= end || qbase + 16 <= head + w.cur) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
            const uint32_t mS = csvEqQuad(q, s4), mQ = csvEqQuad(q, 0x22222222u), mN = csvEqQuad(q, 0x0A0A0A0Au), mR = csvEqQuad(q, 0x0D0D0D0Du);
            for (;;) {  // the quad skip: straight to the next byte this phase cares about
                uint32_t m = w.phase == kCsvUnquoted ? (mS | mQ | mN) : w.phase == kCsvQuoted ? (mQ | mR) : w.phase == kCsvDone ? 0u : 0xFFFFu;
                m &= csvBitRange(int32_t(head + w.cur) - int32_t(qbase), int32_t(end) - int32_t(qbase));
                if (!m) break;
                csvEvent<Trim>(src, sink, w, head, len, sepWord, sepLen, qbase + uint32_t(__builtin_ctz(m)) - head);
            }
        }
    }
    // ---- the value's end
    if (w.phase == kCsvLine) {
        w.status = LC_CSV_EOF;
    } else if (w.phase == kCsvField) {  // behind a separator (or trimmed space): the empty field
        csvEmit(sink, w, len, len, 0);
    } else if (w.phase == kCsvUnquoted) {  // the last line loses one trailing `\r`
        const uint32_t e = (len > w.fb && src.byteAt(head + len - 1) == '\r') ? len - 1 : len;
        csvEmit(sink, w, w.fb, e, 0);
    } else if (w.phase == kCsvQuoted) {
        w.status = LC_CSV_QUOTE;
    } else if (w.phase == kCsvAfterQuote) {
        csvEmit(sink, w, w.fb, len - 1, w.fold);
    }
    *statusOut = uint8_t(w.status);
    *countOut = w.status == LC_CSV_EOF ? 0u : w.nfields;
}

// ---------------------------------------------------------------------------------------------- the host's side
// the text of a field whose span has LC_CSV_FOLD: `""` -> `"`, `\r\n` -> `\n` (raw: the bytes between the field's quotes)
template <class String>
inline String csvFold(const uint8_t* raw, uint32_t n) {
    String out;
    for (uint32_t i = 0; i < n; ++i) {
        if (raw[i] == '"' && i + 1 < n && raw[i + 1] == '"') ++i;
        else if (raw[i] == '\r' && i + 1 < n && raw[i + 1] == '\n') continue;
        out.push_back(char(raw[i]));
    }
    return out;
}

// the host's source: a byte pointer; every byte outside the value reads as one of four bytes the routine would react to -- and a read
// of the routine's OWN outside the value (byteAt) is a bug the stand-alone check traps
struct CsvHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    uint8_t junk[4];
    bool strayRead = false;
    CsvHostSource(const uint8_t* l, uint32_t n, uint32_t head, const CsvConfig& c) : line(l), len(n), headBytes(head & 15u) {
        junk[0] = uint8_t(c.sepWord & 0xFFu), junk[1] = '"', junk[2] = '\n', junk[3] = '\r';
    }
    uint32_t head() const { return headBytes; }
    uint32_t pad(uint32_t p) const { return (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : junk[p & 3u]; }
    uint32_t byteAt(uint32_t p) const {
        if (p < headBytes || p >= headBytes + len) const_cast<CsvHostSource*>(this)->strayRead = true;
        return pad(p);
    }
    uint32_t stageCount(uint32_t end) const { return (end + kCsvStageBytes - 1) / kCsvStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kCsvStageBytes + k * 16;
        for (int t = 0; t < 4; ++t) q[t] = 0;
        for (uint32_t j = 0; j < 16; ++j) q[j >> 2] |= pad(p16 + j) << ((j & 3) * 8);
    }
};

struct CsvHostSink {
    int32_t* rows;  // int32[W][2]
    uint32_t W;
    void field(uint32_t k, int32_t b, int32_t e) {
        if (k < W) rows[k * 2] = b, rows[k * 2 + 1] = e;
    }
};

// one value on the host, placed `head` bytes behind a 16-byte boundary; false: the routine asked for a byte outside the value
inline bool csvReadRecordHost(const CsvConfig& c, const uint8_t* line, uint32_t len, uint32_t head, int32_t* rows, uint32_t W, uint8_t* status,
                              uint32_t* count) {
    CsvHostSource src(line, len, head, c);
    CsvHostSink sink{rows, W};
    if (c.trim) csvReadRecord<true>(src, sink, len, c.sepWord, c.sepLen, status, count);
    else csvReadRecord<false>(src, sink, len, c.sepWord, c.sepLen, status, count);
    return !src.strayRead;
}
