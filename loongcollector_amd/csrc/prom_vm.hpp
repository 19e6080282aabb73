// prom_vm.hpp -- the per-line routine of the Prometheus text-line parser, ONE function for the host and the device.
//
//   promParseLine()   TextParser::ParseLine: HandleStart .. HandleTimestamp, SkipLeadingWhitespace, IsValidNumberChar
//                     (core/prometheus/labels/TextParser.cpp:34-39, 69-335), restated as a byte-at-a-time machine
//   promFinishHost()  host only: the tokens the machine did not decide, through std::strtod as StringTo<double> does
//                     (core/common/StringTools.h:322-342), and the timestamp rules of TextParser.cpp:300-316
//   promUnescape()    host only: the text of an escaped label value by the reference's rule (:171-199), quirk included
//
// The bytes come from a SOURCE in tile coordinates, as in clog_vm.hpp / apsara_vm.hpp: position 0 is the 16-byte boundary at or below
// the line's first byte, the line occupies [head, head + len) and is walked ONCE in 64-byte stages.
//
//   struct Source { uint32_t head() const; uint32_t stageCount(uint32_t end); void stage(uint32_t s); void rowQuad(uint32_t k, uint32_t q[4]); };
//   struct Sink   { void label(uint32_t k, int32_t nb, int32_t ne, int32_t vb, int32_t ve); }   // label k of the line, vb carries the escaped bit
//
// What the reference does, not what the exposition format says: isalpha / isdigit are ASCII here (a byte >= 0x80 is neither); the
// meaning of an escape is picked from the SECOND byte of the label value (mLine[lPos + 1], :181), not from the byte behind the
// backslash -- so the machine only has to skip the byte behind a backslash and remember that there was one; the host rewrites.
//
// Numbers.  The machine converts a token itself only where ONE correctly rounded IEEE operation gives strtod's answer (Clinger's fast
// path): optional sign, decimal digits with an optional point, optional e/E exponent; the digits (leading zeros and the
// point removed) form an integer w <= 2^53; the decimal exponent after moving the point lies in [-22, 22].  The value is w * 10^e or
// w / 10^-e with the power of ten exact.  Also: zero in either sign (any exponent), and inf / infinity / nan in any letter case with an
// optional sign.  EVERY other token -- longer mantissas, other exponents, hex floats, malformed ones -- is left to the host:
// LC_PROM_VALUE_HOST / LC_PROM_TIME_HOST and the token's span.  A timestamp is converted here only when it is a plain digit string
// below 2^53.  This translation unit must be compiled without fast-math; the one operation cannot be contracted with anything.
#pragma once

#include <errno.h>
#include <stdint.h>
#include <stdlib.h>

#include <cmath>
#include <string>

#include "../../include/lc_prom.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_PROM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_PROM_HD inline
#endif

constexpr uint32_t kPromStageBytes = 64;
constexpr uint64_t kPromTwo53 = 1ull << 53;
constexpr int32_t kPromExponentBound = 22;  // 10^22 is the largest power of ten a double holds exactly

struct PromSpan {
    int32_t begin, end;
};
struct PromLine {
    uint8_t status, flags;
    PromSpan name, valueSpan, timeSpan;
    uint64_t value;  // bits
    int64_t secs;
    uint32_t nanos, nlabels;
};

LC_PROM_HD void promClear(PromLine& r) {
    r.status = LC_PROM_OK;
    r.flags = 0;
    r.name = r.valueSpan = r.timeSpan = PromSpan{0, 0};
    r.value = 0;
    r.secs = 0;
    r.nanos = 0;
    r.nlabels = 0;
}

// ASCII only, whatever the locale (a byte >= 0x80 is neither)
LC_PROM_HD bool promIsAlpha(uint32_t c) { return (c | 0x20u) - 'a' < 26u; }
LC_PROM_HD bool promIsDigit(uint32_t c) { return c - '0' < 10u; }
LC_PROM_HD bool promIsBlank(uint32_t c) { return c == ' ' || c == '\t'; }
// IsValidNumberChar :34-39: 0-9 . - + e E I N F T Y i n f t y X x A a
LC_PROM_HD bool promIsNumberChar(uint32_t c) {
    if (promIsDigit(c) || c == '.' || c == '-' || c == '+') return true;
    const uint32_t l = c | 0x20u;
    return c < 0x80u && (l == 'e' || l == 'i' || l == 'n' || l == 'f' || l == 't' || l == 'y' || l == 'x' || l == 'a');
}

// the exact powers of ten (a table in constant memory once compiled)
LC_PROM_HD double promPow10(uint32_t e) {
    switch (e) {
        case 0: return 1e0;
        case 1: return 1e1;
        case 2: return 1e2;
        case 3: return 1e3;
        case 4: return 1e4;
        case 5: return 1e5;
        case 6: return 1e6;
        case 7: return 1e7;
        case 8: return 1e8;
        case 9: return 1e9;
        case 10: return 1e10;
        case 11: return 1e11;
        case 12: return 1e12;
        case 13: return 1e13;
        case 14: return 1e14;
        case 15: return 1e15;
        case 16: return 1e16;
        case 17: return 1e17;
        case 18: return 1e18;
        case 19: return 1e19;
        case 20: return 1e20;
        case 21: return 1e21;
        default: return 1e22;
    }
}
LC_PROM_HD uint64_t promDoubleBits(double v) {
    union {
        double d;
        uint64_t u;
    } x;
    x.d = v;
    return x.u;
}

// ---------------------------------------------------------------------------------------------- a number token, byte by byte
enum : uint32_t { kNumStart = 0, kNumSigned, kNumInt, kNumFrac, kNumExpMark, kNumExpSigned, kNumExp, kNumLetters, kNumHost };
struct PromNumber {
    uint64_t w = 0;        // the digits as an integer (stops growing above 2^53: tooWide)
    uint64_t letters = 0;  // a special spelling, lower case, low byte first
    uint32_t phase = kNumStart, nLetters = 0;
    int32_t frac = 0, exp = 0;
    bool negative = false, expNegative = false, anyDigit = false, tooWide = false;
};

LC_PROM_HD void promNumberStep(PromNumber& n, uint32_t c) {
    const uint32_t l = c | 0x20u;
    switch (n.phase) {
        case kNumStart:
            if (c == '+' || c == '-') {
                n.negative = c == '-';
                n.phase = kNumSigned;
                return;
            }
            [[fallthrough]];
        case kNumSigned:
            if (promIsDigit(c) || c == '.') {
                n.phase = kNumInt;
                break;  // (the byte is the integer part's)
            }
            if (l == 'i' || l == 'n') {
                n.phase = kNumLetters;
                n.letters = l;
                n.nLetters = 1;
                return;
            }
            n.phase = kNumHost;
            return;
        case kNumLetters:
            if (promIsAlpha(c) && n.nLetters < 8) n.letters |= uint64_t(l) << (8 * n.nLetters++);
            else n.phase = kNumHost;
            return;
        default:
            break;
    }
    switch (n.phase) {
        case kNumInt:
        case kNumFrac:
            if (promIsDigit(c)) {
                n.anyDigit = true;
                if (n.w > kPromTwo53) n.tooWide = true;
                else n.w = n.w * 10 + (c - '0');
                if (n.phase == kNumFrac) ++n.frac;
            } else if (c == '.' && n.phase == kNumInt) {
                n.phase = kNumFrac;
            } else if (l == 'e' && n.anyDigit) {
                n.phase = kNumExpMark;
            } else {
                n.phase = kNumHost;
            }
            return;
        case kNumExpMark:
            if (c == '+' || c == '-') {
                n.expNegative = c == '-';
                n.phase = kNumExpSigned;
                return;
            }
            [[fallthrough]];
        case kNumExpSigned:
        case kNumExp:
            if (promIsDigit(c)) {
                if (n.exp < 100000) n.exp = n.exp * 10 + int32_t(c - '0');
                n.phase = kNumExp;
            } else {
                n.phase = kNumHost;
            }
            return;
        default:
            return;
    }
}
// the token's end: true and the bits when the machine decides, false when the host has to
LC_PROM_HD bool promNumberFinish(const PromNumber& n, uint64_t& bits) {
    const uint64_t sign = n.negative ? 0x8000000000000000ull : 0ull;
    if (n.phase == kNumLetters) {
        const bool inf = (n.nLetters == 3 && n.letters == 0x666E69ull) || (n.nLetters == 8 && n.letters == 0x7974696E69666E69ull);
        const bool nan = n.nLetters == 3 && n.letters == 0x6E616Eull;
        if (!inf && !nan) return false;
        bits = sign | (inf ? 0x7FF0000000000000ull : 0x7FF8000000000000ull);
        return true;
    }
    const bool wellFormed = ((n.phase == kNumInt || n.phase == kNumFrac) && n.anyDigit) || n.phase == kNumExp;
    if (!wellFormed || n.tooWide || n.w > kPromTwo53) return false;
    if (n.w == 0) {
        bits = sign;
        return true;
    }
    const int32_t e10 = (n.expNegative ? -n.exp : n.exp) - n.frac;
    if (e10 < -kPromExponentBound || e10 > kPromExponentBound) return false;
    const double w = double(n.w);  // exact: w <= 2^53
    const double v = e10 >= 0 ? w * promPow10(uint32_t(e10)) : w / promPow10(uint32_t(-e10));
    bits = sign | promDoubleBits(v);
    return true;
}

// :300-316 on a millisecond count the machine holds as an integer below 2^53 (every step is exact in a double too)
LC_PROM_HD void promTimestampFromInteger(uint64_t ms, PromLine& out) {
    if (ms < (1ull << 31)) ms *= 1000;
    const int64_t secs = int64_t(ms / 1000);
    if (secs < 1000000000) {
        out.status = LC_PROM_FAIL_TIMESTAMP_SMALL;
        return;
    }
    out.secs = secs;
    out.nanos = uint32_t(ms % 1000) * 1000000u;
    out.flags |= LC_PROM_HAS_TIME;
}

// ---------------------------------------------------------------------------------------------- the line
enum : uint32_t { kPromStart = 0, kPromName, kPromAfterName, kPromLabelStart, kPromLabelName, kPromBeforeEqual, kPromAfterEqual, kPromLabelValue,
                  kPromLabelEscape, kPromAfterLabelValue, kPromBeforeValue, kPromValue, kPromAfterValue, kPromTime, kPromDone, kPromFail };

struct PromWalk {
    uint32_t state = kPromStart;
    uint32_t nameBegin = 0, labelBegin = 0, labelEnd = 0, valueBegin = 0, tokenBegin = 0;
    bool escaped = false, timeDigits = true, timeWide = false;
    uint64_t timeValue = 0;
    PromNumber number;
};

LC_PROM_HD void promFail(PromWalk& w, PromLine& out, uint32_t status) {
    w.state = kPromFail;
    out.status = uint8_t(status);
}
// the value token [tokenBegin, end) is complete
LC_PROM_HD void promValueEnd(PromWalk& w, PromLine& out, uint32_t end) {
    out.valueSpan = PromSpan{int32_t(w.tokenBegin), int32_t(end)};
    if (end == w.tokenBegin) {  // StringTo of an empty string :324
        promFail(w, out, LC_PROM_FAIL_VALUE);
        return;
    }
    uint64_t bits = 0;
    if (promNumberFinish(w.number, bits)) out.value = bits;
    else out.flags |= LC_PROM_VALUE_HOST;
    w.state = kPromAfterValue;
}
LC_PROM_HD void promTimeEnd(PromWalk& w, PromLine& out, uint32_t end) {
    out.timeSpan = PromSpan{int32_t(w.tokenBegin), int32_t(end)};
    w.state = kPromDone;
    if (w.timeDigits && !w.timeWide && w.timeValue < kPromTwo53) promTimestampFromInteger(w.timeValue, out);
    else out.flags |= LC_PROM_TIME_HOST;
    if (out.status != LC_PROM_OK) w.state = kPromFail;
}

// line byte i
template <class Sink>
LC_PROM_HD void promStep(PromWalk& w, Sink& sink, PromLine& out, uint32_t c, uint32_t i, uint32_t size, bool honor) {
    switch (w.state) {
        case kPromStart:  // HandleStart :86-94
            if (promIsBlank(c)) return;
            if (!(promIsAlpha(c) || c == '_' || c == ':')) return promFail(w, out, LC_PROM_FAIL_NAME);
            w.nameBegin = i;
            w.state = kPromName;
            return;
        case kPromName:  // HandleMetricName :97-118
            if (promIsAlpha(c) || c == '_' || c == ':' || promIsDigit(c)) return;
            out.name = PromSpan{int32_t(w.nameBegin), int32_t(i)};
            w.state = kPromAfterName;
            [[fallthrough]];
        case kPromAfterName:
            if (promIsBlank(c)) return;
            if (c == '{') {
                w.state = kPromLabelStart;
                return;
            }
            w.state = kPromBeforeValue;
            break;  // (the byte is the value's)
        case kPromLabelStart:  // HandleLabelName :121-146
            if (promIsBlank(c)) return;
            if (promIsAlpha(c) || c == '_') {
                w.labelBegin = i;
                w.state = kPromLabelName;
            } else if (c == '}') {
                w.state = kPromBeforeValue;
            } else {
                promFail(w, out, LC_PROM_FAIL_LABEL_NAME);
            }
            return;
        case kPromLabelName:
            if (promIsAlpha(c) || c == '_' || promIsDigit(c)) return;
            w.labelEnd = i;
            w.state = kPromBeforeEqual;
            [[fallthrough]];
        case kPromBeforeEqual:
            if (promIsBlank(c)) return;
            if (c != '=') return promFail(w, out, LC_PROM_FAIL_EQUAL);
            w.state = kPromAfterEqual;
            return;
        case kPromAfterEqual:  // HandleEqualSign :149-156
            if (promIsBlank(c)) return;
            if (c != '"') return promFail(w, out, LC_PROM_FAIL_QUOTE);
            w.valueBegin = i + 1;
            w.escaped = false;
            w.state = kPromLabelValue;
            return;
        case kPromLabelValue:  // HandleLabelValue :159-221
            if (c == '"') {
                sink.label(out.nlabels, int32_t(w.labelBegin), int32_t(w.labelEnd), int32_t(w.valueBegin | (w.escaped ? LC_PROM_LABEL_ESCAPED : 0u)),
                           int32_t(i));
                ++out.nlabels;
                w.state = kPromAfterLabelValue;
            } else if (c == '\\') {
                w.escaped = true;
                out.flags |= LC_PROM_ANY_ESCAPE;
                // :177: the byte behind the backslash is consumed with it -- unless the backslash is the line's last byte (:195-197: the
                // reference reads mLine[size] there; not read here, the line fails at its end either way)
                if (i + 1 < size) w.state = kPromLabelEscape;
            }
            return;
        case kPromLabelEscape:
            w.state = kPromLabelValue;
            return;
        case kPromAfterLabelValue:  // :215-220, HandleCommaOrCloseBrace :225-238
            if (promIsBlank(c)) return;
            if (c == ',') w.state = kPromLabelStart;
            else if (c == '}') w.state = kPromBeforeValue;
            else promFail(w, out, LC_PROM_FAIL_LABEL_VALUE_NEXT);
            return;
        default:
            break;
    }
    switch (w.state) {
        case kPromBeforeValue:  // (the blanks behind '}'; behind the name they are gone already)
            if (promIsBlank(c)) return;
            w.tokenBegin = i;
            w.state = kPromValue;
            [[fallthrough]];
        case kPromValue:  // HandleSampleValue :241-271
            if (promIsNumberChar(c)) {
                promNumberStep(w.number, c);
                return;
            }
            if (!promIsBlank(c) && c != '#') return promFail(w, out, LC_PROM_FAIL_VALUE_END);
            promValueEnd(w, out, i);
            if (w.state != kPromAfterValue) return;
            [[fallthrough]];
        case kPromAfterValue:
            if (promIsBlank(c)) return;
            if (c == '#' || !honor) {
                w.state = kPromDone;
                return;
            }
            w.tokenBegin = i;
            w.state = kPromTime;
            [[fallthrough]];
        case kPromTime:  // HandleTimestamp :275-324
            if (promIsNumberChar(c)) {
                if (promIsDigit(c)) {
                    if (w.timeValue >= kPromTwo53) w.timeWide = true;
                    else w.timeValue = w.timeValue * 10 + (c - '0');
                } else {
                    w.timeDigits = false;
                }
                return;
            }
            if (!promIsBlank(c) && c != '#') return promFail(w, out, LC_PROM_FAIL_TIME_END);
            promTimeEnd(w, out, i);
            return;
        default:
            return;
    }
}

// the line's end, met in state w.state
LC_PROM_HD void promEnd(PromWalk& w, PromLine& out, uint32_t size) {
    switch (w.state) {
        case kPromStart: return promFail(w, out, LC_PROM_FAIL_NAME);  // c = '\0' :88
        case kPromName:
            out.name = PromSpan{int32_t(w.nameBegin), int32_t(size)};
            [[fallthrough]];
        case kPromAfterName: return promFail(w, out, LC_PROM_FAIL_NAME_END);
        case kPromLabelStart: return promFail(w, out, LC_PROM_FAIL_LABEL_NAME);  // c = '\0' :122
        case kPromLabelName:
        case kPromBeforeEqual: return promFail(w, out, LC_PROM_FAIL_EQUAL);
        case kPromAfterEqual: return promFail(w, out, LC_PROM_FAIL_QUOTE);
        case kPromLabelValue:
        case kPromLabelEscape: return promFail(w, out, LC_PROM_FAIL_LABEL_VALUE_END);
        case kPromAfterLabelValue: return promFail(w, out, LC_PROM_FAIL_LABEL_VALUE_NEXT);
        case kPromBeforeValue:
            w.tokenBegin = size;
            [[fallthrough]];
        case kPromValue:
            promValueEnd(w, out, size);
            if (w.state == kPromAfterValue) w.state = kPromDone;
            return;
        case kPromAfterValue:
            w.state = kPromDone;
            return;
        case kPromTime: return promTimeEnd(w, out, size);
        default: return;
    }
}

template <class Source, class Sink>
LC_PROM_HD void promParseLine(Source& src, Sink& sink, uint32_t len, bool honor, PromLine& out) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;
    PromWalk w;
    promClear(out);
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kPromStageBytes;
        if (base >= end || w.state >= kPromDone) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kPromStageBytes / 16 && w.state < kPromDone; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
            // ONE copy of the machine: the byte is picked with selects (q[] stays in registers), the loop is not unrolled
#pragma unroll 1
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t p = qbase + j;
                if (p < head || p >= end || w.state >= kPromDone) continue;
                const uint32_t d = j >> 2;
                const uint32_t word = d == 0 ? q[0] : d == 1 ? q[1] : d == 2 ? q[2] : q[3];
                promStep(w, sink, out, (word >> ((j & 3u) * 8)) & 0xFFu, p - head, len, honor);
            }
        }
    }
    if (w.state < kPromDone) promEnd(w, out, len);
    if (out.status != LC_PROM_OK) {
        // a failed line reports its status, the labels it had and nothing else -- but a line that failed BEHIND a value token the
        // machine left open keeps LC_PROM_VALUE_HOST and the span: the reference meets "invalid sample value" first
        out.flags = out.status >= LC_PROM_FAIL_TIME_END ? uint8_t(out.flags & LC_PROM_VALUE_HOST) : uint8_t(0);
        out.value = 0;
        out.secs = 0;
        out.nanos = 0;
    }
}

// ---------------------------------------------------------------------------------------------- the host's source, sink and finish
// a byte pointer; every byte outside the line reads as junk the machine would react to (quote, backslash, brace)
struct PromHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    PromHostSource(const uint8_t* l, uint32_t n, uint32_t head) : line(l), len(n), headBytes(head & 15u) {}
    uint32_t head() const { return headBytes; }
    uint32_t stageCount(uint32_t end) const { return (end + kPromStageBytes - 1) / kPromStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const {
        const uint32_t p16 = stageNow * kPromStageBytes + k * 16;
        for (int d = 0; d < 4; ++d) q[d] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = p16 + j;
            const uint32_t b = (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : (j % 3 == 0 ? uint32_t('"') : j % 3 == 1 ? uint32_t('\\') : uint32_t('}'));
            q[j >> 2] |= b << ((j & 3) * 8);
        }
    }
};
// labels: int32[W][4]
struct PromHostSink {
    int32_t* labels;
    uint32_t W;
    void label(uint32_t k, int32_t nb, int32_t ne, int32_t vb, int32_t ve) {
        if (k >= W) return;
        int32_t* at = labels + size_t(k) * 4;
        at[0] = nb, at[1] = ne, at[2] = vb, at[3] = ve;
    }
};

inline void promParseLineHost(const uint8_t* line, uint32_t len, bool honor, int32_t* labels, uint32_t W, PromLine& out, uint32_t head = 0) {
    PromHostSource src(line, len, head);
    PromHostSink sink{labels, W};
    promParseLine(src, sink, len, honor, out);
}

// StringTo<double> :322-342 over line[span): the whole token, no ERANGE
inline bool promStrtod(const uint8_t* line, PromSpan span, double& v) {
    if (span.end <= span.begin) return false;
    const std::string token(reinterpret_cast<const char*>(line) + span.begin, size_t(span.end - span.begin));
    errno = 0;
    char* stop = nullptr;
    v = std::strtod(token.c_str(), &stop);
    return stop == token.c_str() + token.size() && errno != ERANGE;
}
// the tokens the machine left open; returns how many.  The value is checked first, as the reference meets it first.
inline uint32_t promFinishHost(const uint8_t* line, PromLine& r) {
    if (r.status != LC_PROM_OK) {
        // failed behind an open value token: "invalid sample value" comes first when the token is no number
        double v = 0;
        if (!(r.flags & LC_PROM_VALUE_HOST)) return 0;
        if (!promStrtod(line, r.valueSpan, v)) r.status = LC_PROM_FAIL_VALUE;
        return 1;
    }
    uint32_t finished = 0;
    const auto fail = [&](uint8_t status) {
        r.status = status;
        r.flags &= uint8_t(LC_PROM_VALUE_HOST | LC_PROM_TIME_HOST);
        r.value = 0;
        r.secs = 0;
        r.nanos = 0;
    };
    if (r.flags & LC_PROM_VALUE_HOST) {
        ++finished;
        double v = 0;
        if (!promStrtod(line, r.valueSpan, v)) {
            fail(LC_PROM_FAIL_VALUE);
            return finished;
        }
        r.value = promDoubleBits(v);
    }
    if (r.flags & LC_PROM_TIME_HOST) {
        ++finished;
        double ms = 0;
        if (!promStrtod(line, r.timeSpan, ms)) fail(LC_PROM_FAIL_TIMESTAMP);
        else if (std::isnan(ms)) fail(LC_PROM_FAIL_TIMESTAMP_NAN);  // DEFINED (lc_prom.h)
        else if (ms > 9223372036854775808.0) fail(LC_PROM_FAIL_TIMESTAMP_OVERFLOW);  // :300
        else {
            if (ms < 2147483648.0) ms *= 1000;  // :305
            // :308: outside int64_t the cast is undefined; DEFINED as the failure x86-64's INT64_MIN leads to
            if (!(ms >= -9223372036854775808.0 && ms < 9223372036854775808.0)) {
                fail(LC_PROM_FAIL_TIMESTAMP_SMALL);
            } else {
                const int64_t t = int64_t(ms);
                if (t / 1000 < 1000000000) {
                    fail(LC_PROM_FAIL_TIMESTAMP_SMALL);
                } else {
                    r.secs = t / 1000;
                    r.nanos = uint32_t(t % 1000) * 1000000u;
                    r.flags |= LC_PROM_HAS_TIME;
                }
            }
        }
    }
    return finished;
}
// the text of the escaped label value line[vb, ve): :171-199.  The escape's meaning comes from the value's SECOND byte.
inline void promUnescape(const uint8_t* line, int32_t vb, int32_t ve, std::string& out) {
    out.clear();
    for (int32_t p = vb; p < ve;) {
        if (line[p] != '\\') {
            out.push_back(char(line[p++]));
            continue;
        }
        switch (line[vb + 1]) {  // (p + 1 <= ve: the closing quote stands at ve)
            case '\\':
            case '"': out.push_back(char(line[p + 1])); break;
            case 'n': out.push_back('\n'); break;
            default:
                out.push_back('\\');
                out.push_back(char(line[p + 1]));
                break;
        }
        p += 2;
    }
}
