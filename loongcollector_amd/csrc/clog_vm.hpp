// clog_vm.hpp -- the per-line routines of the container stdout parser, each ONE function for the host and the device.
//
//   clogParseContainerd()   ParseContainerdTextLogLine up to the call of ResetContainerdTextLog
//                           (core/plugin/processor/inner/ProcessorParseContainerLogNative.cpp:176-257)
//   clogParseDocker()       ParseDockerLog, parseLogType, parseValue (:259-462), the "\u" conversion included
//
// The bytes come from a SOURCE in tile coordinates, as in apsara_vm.hpp: position 0 is the 16-byte boundary at or below the line's first
// byte, the line occupies [head, head + len) and is walked ONCE in 64-byte stages.
//
//   struct Source {
//       uint32_t head() const;                     // 0..15
//       uint32_t stageCount(uint32_t end);         // 64-byte stages for a line that ends at tile position end (the device: of the wavefront)
//       void stage(uint32_t s);                    // make stage s current
//       void rowQuad(uint32_t k, uint32_t q[4]);   // quad k (0..3) of the current stage of THIS line
//       uint32_t byteAt(uint32_t p) const;         // one byte of the line at tile position p, out of order (Docker: the last byte)
//       bool anyLane(bool mine) const;             // does any line that is walked together with this one say so (the host: mine)
//   };
//   struct Sink { void put(uint32_t pos, uint32_t byte); }   // the unescaped text, pos relative to the line's first byte
//
// containerd reads the header only: it stops behind the byte two behind the second blank (the tag rule looks no further), so the trip
// count follows where that byte lies and not the line's length.
//
// Docker is the reference's index walk restated as a byte-at-a-time machine.  What the reference looks ahead for is decided from the
// position alone (the key names under `idx + len < size`, "\u" under `idx + 4 < size`), and `buffer[size - 1] == '}'` -- the reference's
// first test -- is the one byte read out of order.  Every `idx >= size` exit of the reference is "the bytes ran out before the closing
// brace at size - 1 was met": the machine fails when it is not in kDone at the line's end.  The unescaped text never overtakes the
// walk (an escape shrinks), so the host may write it in place: every put() lands at or below the byte that was read last.
#pragma once

#include <stdint.h>

#include "../../include/lc_container_log.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_CLOG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_CLOG_HD inline
#endif

constexpr uint32_t kClogStageBytes = 64;
constexpr uint32_t kClogNone = 0xFFFFFFFFu;

struct ClogSpan {
    int32_t begin, end;
};
struct ClogLine {
    uint8_t status, flags;
    ClogSpan span[3];  // LC_CLOG_SPAN_*
    int32_t rewriteBegin;
};

LC_CLOG_HD void clogClear(ClogLine& r) {
    r.status = LC_CLOG_OK;
    r.flags = 0;
    for (int k = 0; k < 3; ++k) r.span[k] = ClogSpan{0, 0};
    r.rewriteBegin = 0;
}

// byte k of "stdout" / "stderr" (k < 6)
LC_CLOG_HD uint32_t clogStdoutByte(uint32_t k) { return uint32_t((0x74756F647473ull >> (k * 8)) & 0xFFu); }
LC_CLOG_HD uint32_t clogStderrByte(uint32_t k) { return uint32_t((0x727265647473ull >> (k * 8)) & 0xFFu); }

// ---------------------------------------------------------------------------------------------- containerd
struct ClogContainerdWalk {
    uint32_t b1 = kClogNone, b2 = kClogNone;  // the first and the second blank
    uint32_t tag = 0;                          // the byte behind the second blank
    bool isOut = true, isErr = true, third = false, done = false;
};

// line byte i
LC_CLOG_HD void clogContainerdStep(ClogContainerdWalk& w, uint32_t ch, uint32_t i) {
    if (w.b1 == kClogNone) {
        if (ch == ' ') w.b1 = i;  // :183
    } else if (w.b2 == kClogNone) {
        if (ch == ' ') {  // :195
            w.b2 = i;
        } else {  // :205
            const uint32_t k = i - w.b1 - 1;
            w.isOut = w.isOut && k < 6 && ch == clogStdoutByte(k);
            w.isErr = w.isErr && k < 6 && ch == clogStderrByte(k);
        }
    } else if (i == w.b2 + 1) {
        w.tag = ch;  // :227
    } else {
        w.third = ch == ' ';  // :235-236: pch3 == pch2 + 2
        w.done = true;
    }
}

template <class Source>
LC_CLOG_HD void clogParseContainerd(Source& src, uint32_t len, ClogLine& out) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;
    ClogContainerdWalk w;
    clogClear(out);
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        const uint32_t base = s * kClogStageBytes;
        if (!src.anyLane(!w.done && base < end)) break;
        src.stage(s);
        if (w.done || base >= end) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kClogStageBytes / 16 && !w.done; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t p = qbase + j;
                if (p < head || p >= end || w.done) continue;
                clogContainerdStep(w, (q[j >> 2] >> ((j & 3) * 8)) & 0xFFu, p - head);
            }
        }
    }
    if (w.b1 == kClogNone) {
        out.status = LC_CLOG_FAIL_TIME;
        return;
    }
    if (w.b2 == kClogNone) {
        out.status = LC_CLOG_FAIL_SOURCE;
        return;
    }
    out.span[LC_CLOG_SPAN_SOURCE] = ClogSpan{int32_t(w.b1 + 1), int32_t(w.b2)};
    const bool sixBytes = w.b2 - w.b1 - 1 == 6;
    if (!(sixBytes && (w.isOut || w.isErr))) {
        out.status = LC_CLOG_FAIL_STREAM;
        return;
    }
    out.span[LC_CLOG_SPAN_TIME] = ClogSpan{0, int32_t(w.b1)};
    if (w.isErr) out.flags |= LC_CLOG_STDERR;
    // the tag rule: 'P' or 'F' behind the second blank AND the third blank exactly two bytes behind the second (:227-242).  A line that
    // ends at the second blank or at the tag byte has no third blank
    const bool tagged = (w.tag == 'P' || w.tag == 'F') && w.third;
    if (tagged && w.tag == 'P') out.flags |= LC_CLOG_PARTIAL;
    out.span[LC_CLOG_SPAN_CONTENT] = ClogSpan{int32_t(w.b2 + (tagged ? 3u : 1u)), int32_t(len)};
}

// ---------------------------------------------------------------------------------------------- Docker
enum : uint32_t { kDockOpen = 0, kDockTop, kDockKey, kDockKeyQuote, kDockColon, kDockValueQuote, kDockValue, kDockEscape, kDockUnicode, kDockAfter,
                  kDockDone, kDockFail };
enum : uint32_t { kDockLog = 0, kDockStream = 1, kDockTime = 2 };  // DockerLogType, and the order parseLogType tries them in

// byte k of the key name of a type
LC_CLOG_HD uint32_t clogKeyByte(uint32_t type, uint32_t k) {
    const uint64_t name = type == kDockLog ? 0x676F6Cull : type == kDockStream ? 0x6D6165727473ull : 0x656D6974ull;
    return uint32_t((name >> (k * 8)) & 0xFFu);
}
LC_CLOG_HD uint32_t clogKeyLength(uint32_t type) { return type == kDockLog ? 3u : type == kDockStream ? 6u : 4u; }

// std::stoul(four bytes, nullptr, 16): blanks (isspace), a sign, "0x" / "0X", hex digits up to the first other byte.  false: no digit
// (std::invalid_argument).  The bytes are packed low byte first.
LC_CLOG_HD int32_t clogHexDigit(uint32_t c) {
    if (c - '0' < 10u) return int32_t(c - '0');
    if ((c | 0x20u) - 'a' < 6u) return int32_t((c | 0x20u) - 'a' + 10);
    return -1;
}
LC_CLOG_HD uint32_t clogFourByte(uint32_t four, uint32_t k) { return k < 4 ? (four >> (k * 8)) & 0xFFu : 0x100u; }  // (behind the text: no digit, no blank)
LC_CLOG_HD bool clogStoul16(uint32_t four, uint32_t& value, bool& negative) {
    uint32_t at = 0;
    while (at < 4 && (clogFourByte(four, at) == ' ' || clogFourByte(four, at) - 9u < 5u)) ++at;
    negative = false;
    if (clogFourByte(four, at) == '+' || clogFourByte(four, at) == '-') negative = clogFourByte(four, at++) == '-';
    // (the prefix counts only in front of a digit: "0xZZ" is the number 0 that ends at the x)
    if (clogFourByte(four, at) == '0' && (clogFourByte(four, at + 1) | 0x20u) == 'x' && clogHexDigit(clogFourByte(four, at + 2)) >= 0) at += 2;
    value = 0;
    uint32_t digits = 0;
    while (clogHexDigit(clogFourByte(four, at)) >= 0) {
        value = value * 16 + uint32_t(clogHexDigit(clogFourByte(four, at++)));
        ++digits;
    }
    return digits != 0;
}

struct ClogDockerWalk {
    uint32_t state = kDockOpen, type = 0, keyAt = 0, keys = 0;
    uint32_t valueBegin = 0, writeAt = 0;  // endIndex
    uint32_t four = 0, fourCount = 0;
    uint32_t rewrites = 0, firstBackslash = 0;
    bool escaped = false;        // of the value that is walked
    bool winnerEscaped = false;  // of the "log" value that counts
    ClogSpan log{0, 0}, stream{0, 0}, time{0, 0};
    int32_t rewriteBegin = 0;
};

// std::wstring_convert<std::codecvt_utf8<char32_t>>::to_bytes of one value below 0x10000: surrogates are encoded like any other value
template <class Sink>
LC_CLOG_HD void clogPutUtf8(ClogDockerWalk& w, Sink& sink, uint32_t v) {
    if (v < 0x80u) {
        sink.put(w.writeAt++, v);
    } else if (v < 0x800u) {
        sink.put(w.writeAt++, 0xC0u | (v >> 6));
        sink.put(w.writeAt++, 0x80u | (v & 0x3Fu));
    } else {
        sink.put(w.writeAt++, 0xE0u | (v >> 12));
        sink.put(w.writeAt++, 0x80u | ((v >> 6) & 0x3Fu));
        sink.put(w.writeAt++, 0x80u | (v & 0x3Fu));
    }
}

// line byte i of a line of `size` bytes
template <class Sink>
LC_CLOG_HD void clogDockerStep(ClogDockerWalk& w, Sink& sink, uint32_t ch, uint32_t i, uint32_t size) {
    switch (w.state) {
        case kDockOpen:  // :362
            w.state = ch == '{' ? kDockTop : kDockFail;
            return;
        case kDockAfter:  // :429-446: blanks, the comma while fewer than three keys were seen, blanks
            if (ch == ' ') return;
            if (w.keys < 3) {
                w.state = ch == ',' ? kDockTop : kDockFail;
                return;
            }
            w.state = kDockTop;  // (no comma is looked for: this byte is the loop's)
            [[fallthrough]];
        case kDockTop:  // :370-385
            if (ch == ' ') return;
            if (ch == '}') w.state = i == size - 1 ? kDockDone : kDockFail;
            else if (ch == '"') w.state = kDockKey, w.keyAt = 0;
            else w.state = kDockFail;
            return;
        case kDockKey:  // parseLogType :266-292
            if (w.keyAt == 0) {
                w.type = ch == 'l' ? kDockLog : ch == 's' ? kDockStream : kDockTime;
                if (!(i + clogKeyLength(w.type) < size)) {
                    w.state = kDockFail;
                    return;
                }
            }
            if (ch != clogKeyByte(w.type, w.keyAt)) {
                w.state = kDockFail;
                return;
            }
            if (++w.keyAt == clogKeyLength(w.type)) {
                ++w.keys;  // :391
                w.state = kDockKeyQuote;
            }
            return;
        case kDockKeyQuote:  // :394
            w.state = ch == '"' ? kDockColon : kDockFail;
            return;
        case kDockColon:  // :398-407
            if (ch == ' ') return;
            w.state = ch == ':' ? kDockValueQuote : kDockFail;
            return;
        case kDockValueQuote:  // :408-422
            if (ch == ' ') return;
            if (ch != '"') {
                w.state = kDockFail;
                return;
            }
            w.state = kDockValue;
            w.valueBegin = w.writeAt = i + 1;
            w.escaped = false;
            return;
        case kDockValue:  // parseValue :301-358
            if (ch == '"') {
                const ClogSpan value{int32_t(w.valueBegin), int32_t(w.writeAt)};  // :448-458
                if (w.type == kDockStream) w.stream = value;
                if (w.type == kDockTime) w.time = value;
                if (w.type == kDockLog) {
                    w.log = value;
                    w.winnerEscaped = w.escaped;
                    w.rewriteBegin = w.escaped ? int32_t(w.firstBackslash) : 0;
                }
                w.state = kDockAfter;
            } else if (ch == '\\') {
                if (w.type != kDockLog) {  // :304
                    w.state = kDockFail;
                    return;
                }
                if (!w.escaped) {
                    w.escaped = true;
                    w.firstBackslash = i;
                    ++w.rewrites;
                }
                w.state = kDockEscape;
            } else {
                if (w.escaped) sink.put(w.writeAt, ch);  // (in front of the first backslash the byte stands where it is)
                ++w.writeAt;
            }
            return;
        case kDockEscape: {  // :311-351
            uint32_t plain = 0x100u;
            switch (ch) {
                case '"': plain = '"'; break;
                case '\\': plain = '\\'; break;
                case '/': plain = '/'; break;
                case 'b': plain = '\b'; break;
                case 'f': plain = '\f'; break;
                case 'n': plain = '\n'; break;
                case 'r': plain = '\r'; break;
                case 't': plain = '\t'; break;
                default: break;
            }
            w.state = kDockValue;
            if (plain != 0x100u) {
                sink.put(w.writeAt++, plain);
            } else if (ch == 'u' && i + 4 < size) {  // :337
                w.state = kDockUnicode;
                w.four = 0;
                w.fourCount = 0;
            } else {
                sink.put(w.writeAt++, '\\');
                sink.put(w.writeAt++, ch);
            }
            return;
        }
        case kDockUnicode: {  // :338-345
            w.four |= ch << (w.fourCount * 8);
            if (++w.fourCount < 4) return;
            uint32_t value = 0;
            bool negative = false;
            // no digit: stoul throws; a negative number other than zero wraps above 0x10FFFF: to_bytes throws.  DEFINED: the line fails
            if (!clogStoul16(w.four, value, negative) || (negative && value != 0)) {
                w.state = kDockFail;
                return;
            }
            clogPutUtf8(w, sink, value);
            w.state = kDockValue;
            return;
        }
        default:
            return;
    }
}

// stream: the bytes of the stream value that decide stdout / stderr are read again from the source (at most six)
template <class Source, class Sink>
LC_CLOG_HD void clogParseDocker(Source& src, Sink& sink, uint32_t len, ClogLine& out) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;
    ClogDockerWalk w;
    clogClear(out);
    // :362: the first test the reference makes, before it writes anything
    if (len == 0 || src.byteAt(end - 1) != '}') w.state = kDockFail;
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kClogStageBytes;
        if (base >= end || w.state >= kDockDone) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kClogStageBytes / 16 && w.state < kDockDone; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t p = qbase + j;
                if (p < head || p >= end || w.state >= kDockDone) continue;
                clogDockerStep(w, sink, (q[j >> 2] >> ((j & 3) * 8)) & 0xFFu, p - head, len);
            }
        }
    }
    if (w.rewrites) out.flags |= LC_CLOG_ESCAPED;
    if (w.state != kDockDone) {
        out.status = LC_CLOG_FAIL_JSON;
        if (w.rewrites) out.flags |= LC_CLOG_REPLAY;
        return;
    }
    if (w.rewrites > 1 || (w.rewrites == 1 && !w.winnerEscaped)) out.flags |= LC_CLOG_REPLAY;
    out.span[LC_CLOG_SPAN_TIME] = w.time;
    out.span[LC_CLOG_SPAN_SOURCE] = w.stream;
    out.span[LC_CLOG_SPAN_CONTENT] = w.log;
    if (!(out.flags & LC_CLOG_REPLAY)) out.rewriteBegin = w.rewriteBegin;
    // :484: stdout or stderr.  (A stream value holds no escape, so its bytes are the source's.)
    const ClogSpan st = w.stream;
    bool isOut = st.end - st.begin == 6, isErr = isOut;
    for (uint32_t k = 0; k < 6 && (isOut || isErr); ++k) {
        const uint32_t b = src.byteAt(head + uint32_t(st.begin) + k);
        isOut = isOut && b == clogStdoutByte(k);
        isErr = isErr && b == clogStderrByte(k);
    }
    if (!(isOut || isErr)) out.status = LC_CLOG_FAIL_STREAM;
    else if (isErr) out.flags |= LC_CLOG_STDERR;
}

// ---------------------------------------------------------------------------------------------- the host's source and sinks
// a byte pointer; every byte outside the line reads as junk the machines would react to (blank, quote, backslash)
struct ClogHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    ClogHostSource(const uint8_t* l, uint32_t n, uint32_t head) : line(l), len(n), headBytes(head & 15u) {}
    uint32_t head() const { return headBytes; }
    uint32_t stageCount(uint32_t end) const { return (end + kClogStageBytes - 1) / kClogStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    bool anyLane(bool mine) const { return mine; }
    uint32_t byteAt(uint32_t p) const { return line[p - headBytes]; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kClogStageBytes + k * 16;
        for (int d = 0; d < 4; ++d) q[d] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = p16 + j;
            const uint32_t b = (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : (j % 3 == 0 ? uint32_t(' ') : j % 3 == 1 ? uint32_t('"') : uint32_t('\\'));
            q[j >> 2] |= b << ((j & 3) * 8);
        }
    }
};
// in place, as the reference writes; or into a shadow of the line (the device's contract)
struct ClogByteSink {
    uint8_t* at;
    void put(uint32_t pos, uint32_t byte) { at[pos] = uint8_t(byte); }
};

inline void clogParseContainerdHost(const uint8_t* line, uint32_t len, ClogLine& out, uint32_t head = 0) {
    ClogHostSource src(line, len, head);
    clogParseContainerd(src, len, out);
}
// shadow: where the unescaped text goes, indexed like the line; the line itself for the reference's in-place rewrite
inline void clogParseDockerHost(const uint8_t* line, uint32_t len, uint8_t* shadow, ClogLine& out, uint32_t head = 0) {
    ClogHostSource src(line, len, head);
    ClogByteSink sink{shadow};
    clogParseDocker(src, sink, len, out);
}
