// json_vm.hpp -- the per-line routine of the JSON parser, ONE function for the host and the device.
//
// jsonWalkLine() does for one line what ProcessorParseJsonNative::JsonLogLineParserSimdJson does before it touches the event
// (core/plugin/processor/ProcessorParseJsonNative.cpp:257-366): it decides whether the line is ONE valid JSON object (strict RFC 8259
// over valid UTF-8, the whole document validated, at most 1024 levels: tests/golden/README_json.md) and reports every top-level member
// as a record (lc_json_member_t, include/lc_json.h).  It is a pushdown walk, one byte at a time, whose whole state lives in
// registers, so that every token may straddle a stage boundary: the grammar position, the nesting stack (one bit per level: object or
// array), the escape under way (hex digits left, the code unit, a pending high surrogate), the UTF-8 sequence under way (bytes left
// and the bounds of the next one), the rest of a literal, and the number's sign, digits and overflow.
//
// Bytes come from a SOURCE in "tile coordinates", as for delimSplitLine (delim_vm.hpp):
//   struct Source {
//       uint32_t head() const;                          // 0..15
//       uint32_t stageCount(uint32_t end);              // 64-byte stages for a line that ends at tile position end (the device: of the WAVEFRONT)
//       void stage(uint32_t s);                         // make stage s current
//       void rowQuad(uint32_t k, uint32_t q[4]);        // quad k (0..3) of the current stage of THIS line
//       uint32_t byteAt(uint32_t p) const;              // one byte of the line at tile position p, for the re-read below
//   };
// DEEP = false keeps levels 0..63 in two registers and ends a line that goes deeper with LC_JSON_DEEP; DEEP = true keeps 1024 bits in
// `deep` (32 words of the caller's).
//
// Unescaping: text is a view of the line until its first backslash.  There the routine copies what it has passed of the string into
// `shadow` (the line's own bytes of the shadow buffer; the one re-read of the source, byteAt) and from then on writes every unescaped
// byte behind it, so that shadow[begin .. begin + unescaped length) is the text; the span's begin gets LC_JSON_ESCAPED and its end is
// begin + the unescaped length.  Only top-level keys and string values are written; nested strings are validated only.
#pragma once

#include <stdint.h>

#include "../../include/lc_json.h"

#if defined(__HIPCC__)
#define LC_JSON_HD __host__ __device__ __forceinline__
#else
#define LC_JSON_HD inline
#endif

constexpr uint32_t kJsonStageBytes = 64;
constexpr uint32_t kJsonRegisterLevels = 64;
constexpr uint32_t kJsonDeepWords = LC_JSON_MAX_DEPTH / 32;

enum : uint32_t {
    kJsStart = 0,   // before the root's '{'
    kJsObjFirst,    // behind '{': a key or '}'
    kJsObjKey,      // behind ',' in an object: a key
    kJsColon,       // behind a key
    kJsValue,       // a value must begin
    kJsArrFirst,    // behind '[': a value or ']'
    kJsAfter,       // behind a value: ',' or the closing bracket
    kJsEnd,         // behind the root's '}': blanks only
    kJsStr,
    kJsEsc,         // behind a backslash
    kJsHex,         // inside \uXXXX
    kJsSurBs,       // behind a high surrogate: a backslash must follow
    kJsSurU,        // ... and a 'u'
    kJsUtf8,        // continuation bytes
    kJsLit,
    kJsNumMinus,    // (every state from here on is inside a number)
    kJsNumZero,
    kJsNumInt,
    kJsNumDot,
    kJsNumFrac,
    kJsNumE,
    kJsNumESign,
    kJsNumExp,
};

struct JsonWalk {
    uint32_t st = kJsStart, depth = 0, lo = 0, hi = 0;
    uint32_t kb = 0, ke = 0, vb = 0;  // the top-level member under way (kb, vb: with the flag bit)
    uint32_t sb = 0, wr = 0;          // the current top-level string: its begin, and where the next unescaped byte goes
    uint32_t cp = 0, hexLeft = 0, hiSur = 0;
    uint32_t u8need = 0, u8lo = 0, u8hi = 0;
    uint32_t lit = 0, litType = 0;
    uint64_t acc = 0;
    bool inKey = false, top = false, flagged = false, neg = false, ovf = false, isInt = false;
    uint32_t nmembers = 0, errpos = 0;
    uint8_t status = LC_JSON_OK;
    bool stop = false;
};

LC_JSON_HD void jsonFail(JsonWalk& w, uint32_t p) {
    w.status = LC_JSON_FAIL;
    w.errpos = p;
    w.stop = true;
}

LC_JSON_HD void jsonEmit(JsonWalk& w, uint32_t type, uint32_t vb, uint32_t ve, uint32_t W, lc_json_member_t* row) {
    if (w.nmembers < W) {
        lc_json_member_t m;
        m.key_begin = w.kb;
        m.key_end = w.ke;
        m.val_begin = vb;
        m.val_end = ve;
        m.type = uint8_t(type);
        m.reserved[0] = m.reserved[1] = m.reserved[2] = 0;
        row[w.nmembers] = m;
    }
    ++w.nmembers;
}

template <bool DEEP>
LC_JSON_HD bool jsonTopIsObject(const JsonWalk& w, const uint32_t* deep) {
    const uint32_t i = w.depth - 1;
    if (DEEP) return (deep[i >> 5] >> (i & 31u)) & 1u;
    return ((i < 32 ? w.lo >> i : w.hi >> (i - 32)) & 1u) != 0;
}

template <bool DEEP>
LC_JSON_HD void jsonPush(JsonWalk& w, bool isObject, uint32_t p, uint32_t* deep) {
    const uint32_t i = w.depth;
    if (!DEEP && i == kJsonRegisterLevels) {  // the second launch finishes this line
        w.status = LC_JSON_DEEP;
        w.errpos = p;
        w.stop = true;
        return;
    }
    if (i == LC_JSON_MAX_DEPTH) {
        jsonFail(w, p);
        return;
    }
    const uint32_t bit = 1u << (i & 31u);
    if (DEEP) {
        const uint32_t word = deep[i >> 5];
        deep[i >> 5] = isObject ? (word | bit) : (word & ~bit);
    } else if (i < 32) {
        w.lo = isObject ? (w.lo | bit) : (w.lo & ~bit);
    } else {
        w.hi = isObject ? (w.hi | bit) : (w.hi & ~bit);
    }
    w.depth = i + 1;
}

// a container closes at p with ch ('}' or ']')
LC_JSON_HD void jsonClose(JsonWalk& w, uint32_t ch, uint32_t p, uint32_t W, lc_json_member_t* row) {
    --w.depth;
    if (w.depth == 0) {
        w.st = kJsEnd;
        return;
    }
    if (w.depth == 1) jsonEmit(w, ch == '}' ? LC_JSON_OBJECT : LC_JSON_ARRAY, w.vb, p + 1, W, row);
    w.st = kJsAfter;
}

LC_JSON_HD void jsonPut(JsonWalk& w, uint32_t ch, uint8_t* shadow) {
    if (w.top && w.flagged) shadow[w.wr++] = uint8_t(ch);
}

LC_JSON_HD void jsonPutCodePoint(JsonWalk& w, uint32_t c, uint8_t* shadow) {
    if (c < 0x80) {
        jsonPut(w, c, shadow);
    } else if (c < 0x800) {
        jsonPut(w, 0xC0 | (c >> 6), shadow);
        jsonPut(w, 0x80 | (c & 0x3F), shadow);
    } else if (c < 0x10000) {
        jsonPut(w, 0xE0 | (c >> 12), shadow);
        jsonPut(w, 0x80 | ((c >> 6) & 0x3F), shadow);
        jsonPut(w, 0x80 | (c & 0x3F), shadow);
    } else {
        jsonPut(w, 0xF0 | (c >> 18), shadow);
        jsonPut(w, 0x80 | ((c >> 12) & 0x3F), shadow);
        jsonPut(w, 0x80 | ((c >> 6) & 0x3F), shadow);
        jsonPut(w, 0x80 | (c & 0x3F), shadow);
    }
}

// the number ends in front of position p (a byte that cannot continue it, or the line's end)
LC_JSON_HD void jsonNumberDone(JsonWalk& w, uint32_t p, uint32_t W, lc_json_member_t* row) {
    if (w.depth == 1) {
        // ProcessNumberValueOptimized :157-173: an integer literal that fits int64 (negative) / uint64 is printed as that integer
        const bool fits = w.isInt && !w.ovf && (!w.neg || w.acc <= 0x8000000000000000ull);
        const bool minusZero = fits && w.neg && w.acc == 0;  // "-0" prints "0"
        jsonEmit(w, fits ? LC_JSON_INT : LC_JSON_DOUBLE, minusZero ? w.vb + 1 : w.vb, p, W, row);
    }
    w.st = kJsAfter;
}

// one byte of a number: true = consumed (or failed), false = the number ended in front of it
LC_JSON_HD bool jsonNumberStep(JsonWalk& w, uint32_t ch, uint32_t p) {
    const bool digit = ch - '0' < 10u;
    const bool exp = ch == 'e' || ch == 'E';
    switch (w.st) {
    case kJsNumMinus:
        if (ch == '0') w.st = kJsNumZero;
        else if (digit) {
            w.st = kJsNumInt;
            w.acc = ch - '0';
        } else jsonFail(w, p);
        return true;
    case kJsNumZero:
    case kJsNumInt:
        if (digit && w.st == kJsNumInt) {
            const uint32_t d = ch - '0';
            if (w.acc > 1844674407370955161ull || (w.acc == 1844674407370955161ull && d > 5)) w.ovf = true;
            w.acc = w.acc * 10 + d;
            return true;
        }
        if (ch == '.') {
            w.st = kJsNumDot;
            w.isInt = false;
            return true;
        }
        if (exp) {
            w.st = kJsNumE;
            w.isInt = false;
            return true;
        }
        return false;  // (a digit behind a leading 0 fails as "what follows a value")
    case kJsNumDot:
        if (digit) w.st = kJsNumFrac;
        else jsonFail(w, p);
        return true;
    case kJsNumFrac:
        if (digit) return true;
        if (exp) {
            w.st = kJsNumE;
            return true;
        }
        return false;
    case kJsNumE:
        if (ch == '+' || ch == '-') w.st = kJsNumESign;
        else if (digit) w.st = kJsNumExp;
        else jsonFail(w, p);
        return true;
    case kJsNumESign:
        if (digit) w.st = kJsNumExp;
        else jsonFail(w, p);
        return true;
    default:  // kJsNumExp
        return digit;
    }
}

// one byte ch at line position p
template <bool DEEP, class Source>
LC_JSON_HD void jsonStep(JsonWalk& w, uint32_t ch, uint32_t p, const Source& src, uint8_t* shadow, uint32_t W, lc_json_member_t* row,
                         uint32_t* deep) {
    if (w.st >= kJsNumMinus) {
        if (jsonNumberStep(w, ch, p)) return;
        jsonNumberDone(w, p, W, row);  // ... and ch is what follows a value
    }
    const bool blank = ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r';
    switch (w.st) {
    case kJsStr:
        if (ch == '"') {
            const uint32_t e = w.flagged ? w.wr : p;
            if (w.inKey) {
                if (w.top) {
                    w.ke = e;
                    if (w.flagged) w.kb |= LC_JSON_ESCAPED;
                }
                w.st = kJsColon;
            } else {
                if (w.top) jsonEmit(w, LC_JSON_STRING, w.flagged ? (w.vb | LC_JSON_ESCAPED) : w.vb, e, W, row);
                w.st = kJsAfter;
            }
        } else if (ch == '\\') {
            if (w.top && !w.flagged) {  // the first escape of a top-level text: what has passed of it goes to the shadow
                w.flagged = true;
                const uint32_t head = src.head();
                for (uint32_t i = w.sb; i < p; ++i) shadow[i] = uint8_t(src.byteAt(head + i));
                w.wr = p;
            }
            w.st = kJsEsc;
        } else if (ch < 0x20) {
            jsonFail(w, p);
        } else if (ch < 0x80) {
            jsonPut(w, ch, shadow);
        } else {  // the lead byte of a UTF-8 sequence (Unicode 15 table 3-7)
            if (ch < 0xC2 || ch > 0xF4) {
                jsonFail(w, p);
                return;
            }
            w.u8lo = 0x80;
            w.u8hi = 0xBF;
            if (ch < 0xE0) {
                w.u8need = 1;
            } else if (ch < 0xF0) {
                w.u8need = 2;
                if (ch == 0xE0) w.u8lo = 0xA0;  // no overlong form
                if (ch == 0xED) w.u8hi = 0x9F;  // no encoded surrogate
            } else {
                w.u8need = 3;
                if (ch == 0xF0) w.u8lo = 0x90;
                if (ch == 0xF4) w.u8hi = 0x8F;  // nothing above U+10FFFF
            }
            jsonPut(w, ch, shadow);
            w.st = kJsUtf8;
        }
        return;
    case kJsUtf8:
        if (ch < w.u8lo || ch > w.u8hi) {
            jsonFail(w, p);
            return;
        }
        jsonPut(w, ch, shadow);
        w.u8lo = 0x80;
        w.u8hi = 0xBF;
        if (--w.u8need == 0) w.st = kJsStr;
        return;
    case kJsEsc: {
        uint32_t out;
        switch (ch) {
        case '"': out = '"'; break;
        case '\\': out = '\\'; break;
        case '/': out = '/'; break;
        case 'b': out = 8; break;
        case 'f': out = 12; break;
        case 'n': out = 10; break;
        case 'r': out = 13; break;
        case 't': out = 9; break;
        case 'u':
            w.hexLeft = 4;
            w.cp = 0;
            w.st = kJsHex;
            return;
        default:
            jsonFail(w, p);
            return;
        }
        jsonPut(w, out, shadow);
        w.st = kJsStr;
        return;
    }
    case kJsHex: {
        uint32_t v;
        if (ch - '0' < 10u) v = ch - '0';
        else if ((ch | 0x20) - 'a' < 6u) v = (ch | 0x20) - 'a' + 10;
        else {
            jsonFail(w, p);
            return;
        }
        w.cp = (w.cp << 4) | v;
        if (--w.hexLeft) return;
        if (w.hiSur) {  // the second half of a pair
            if (w.cp < 0xDC00 || w.cp > 0xDFFF) {
                jsonFail(w, p);
                return;
            }
            jsonPutCodePoint(w, 0x10000 + ((w.hiSur - 0xD800) << 10) + (w.cp - 0xDC00), shadow);
            w.hiSur = 0;
            w.st = kJsStr;
        } else if (w.cp >= 0xD800 && w.cp <= 0xDBFF) {
            w.hiSur = w.cp;
            w.st = kJsSurBs;
        } else if (w.cp >= 0xDC00 && w.cp <= 0xDFFF) {
            jsonFail(w, p);  // a low surrogate on its own
        } else {
            jsonPutCodePoint(w, w.cp, shadow);
            w.st = kJsStr;
        }
        return;
    }
    case kJsSurBs:
        if (ch == '\\') w.st = kJsSurU;
        else jsonFail(w, p);
        return;
    case kJsSurU:
        if (ch == 'u') {
            w.hexLeft = 4;
            w.cp = 0;
            w.st = kJsHex;
        } else jsonFail(w, p);
        return;
    case kJsLit:
        if (ch != (w.lit & 0xFFu)) {
            jsonFail(w, p);
            return;
        }
        w.lit >>= 8;
        if (!w.lit) {
            if (w.depth == 1) jsonEmit(w, w.litType, w.vb, p + 1, W, row);
            w.st = kJsAfter;
        }
        return;
    case kJsStart:
        if (blank) return;
        if (ch == '{') {
            jsonPush<DEEP>(w, true, p, deep);
            w.st = kJsObjFirst;
        } else jsonFail(w, p);  // (the root must be an object)
        return;
    case kJsObjFirst:
    case kJsObjKey:
        if (blank) return;
        if (ch == '"') {
            w.inKey = true;
            w.top = w.depth == 1;
            w.flagged = false;
            w.sb = p + 1;
            if (w.top) w.kb = p + 1;
            w.st = kJsStr;
        } else if (ch == '}' && w.st == kJsObjFirst) {
            jsonClose(w, ch, p, W, row);
        } else jsonFail(w, p);
        return;
    case kJsColon:
        if (blank) return;
        if (ch == ':') w.st = kJsValue;
        else jsonFail(w, p);
        return;
    case kJsValue:
    case kJsArrFirst:
        if (blank) return;
        if (w.depth == 1) w.vb = p;
        if (ch == '"') {
            w.inKey = false;
            w.top = w.depth == 1;
            w.flagged = false;
            w.sb = p + 1;
            if (w.top) w.vb = p + 1;
            w.st = kJsStr;
        } else if (ch == '{' || ch == '[') {
            jsonPush<DEEP>(w, ch == '{', p, deep);
            if (!w.stop) w.st = ch == '{' ? kJsObjFirst : kJsArrFirst;
        } else if (ch == '-' || ch - '0' < 10u) {
            w.neg = ch == '-';
            w.ovf = false;
            w.isInt = true;
            w.acc = w.neg ? 0 : ch - '0';
            w.st = w.neg ? kJsNumMinus : ch == '0' ? kJsNumZero : kJsNumInt;
        } else if (ch == 't') {
            w.lit = 'r' | ('u' << 8) | ('e' << 16);
            w.litType = LC_JSON_TRUE;
            w.st = kJsLit;
        } else if (ch == 'f') {
            w.lit = 'a' | ('l' << 8) | ('s' << 16) | (uint32_t('e') << 24);
            w.litType = LC_JSON_FALSE;
            w.st = kJsLit;
        } else if (ch == 'n') {
            w.lit = 'u' | ('l' << 8) | ('l' << 16);
            w.litType = LC_JSON_NULL;
            w.st = kJsLit;
        } else if (ch == ']' && w.st == kJsArrFirst) {
            jsonClose(w, ch, p, W, row);
        } else jsonFail(w, p);
        return;
    case kJsAfter: {
        if (blank) return;
        const bool inObject = jsonTopIsObject<DEEP>(w, deep);
        if (ch == ',') w.st = inObject ? kJsObjKey : kJsValue;
        else if (ch == (inObject ? uint32_t('}') : uint32_t(']'))) jsonClose(w, ch, p, W, row);
        else jsonFail(w, p);
        return;
    }
    default:  // kJsEnd: nothing but blanks behind the root
        if (!blank) jsonFail(w, p);
        return;
    }
}

// W: how many records `row` holds.  shadow: the line's own bytes of the shadow buffer.  deep: 32 words (DEEP only)
template <bool DEEP, class Source>
LC_JSON_HD void jsonWalkLine(Source& src, uint32_t len, uint32_t W, lc_json_member_t* row, uint8_t* shadow, uint32_t* deep, uint8_t* statusOut,
                             uint32_t* nmembersOut, uint32_t* errposOut) {
    const uint32_t head = src.head();
    const uint32_t end = head + len;  // tile position
    JsonWalk w;
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * kJsonStageBytes;
        if (base >= end || w.stop || len == 0) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < kJsonStageBytes / 16; ++k) {
            const uint32_t qbase = base + k * 16;
            if (qbase >= end || qbase + 16 <= head || w.stop) continue;
            uint32_t q[4];
            src.rowQuad(k, q);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                uint32_t word = q[j];
#pragma unroll 1
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t p = qbase + j * 4 + b;
                    if (p >= head && p < end && !w.stop) jsonStep<DEEP>(w, word & 0xFFu, p - head, src, shadow, W, row, deep);
                    word >>= 8;
                }
            }
        }
    }
    if (len == 0) {
        w.status = LC_JSON_EMPTY;
    } else if (!w.stop && w.st != kJsEnd) {
        jsonFail(w, len);  // the line ends inside the document
    }
    *statusOut = w.status;
    *nmembersOut = w.status == LC_JSON_OK ? w.nmembers : 0u;
    *errposOut = w.status == LC_JSON_FAIL || w.status == LC_JSON_DEEP ? w.errpos : 0u;
}

// the host's source: a byte pointer; every byte outside the line reads as junk that would change the answer if it were interpreted
struct JsonHostSource {
    const uint8_t* line;
    uint32_t len, headBytes, stageNow = 0;
    JsonHostSource(const uint8_t* l, uint32_t n, uint32_t head) : line(l), len(n), headBytes(head & 15u) {}
    uint32_t head() const { return headBytes; }
    void quadAt(uint32_t p16, uint32_t q[4]) const {
        for (int k = 0; k < 4; ++k) q[k] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t p = p16 + j;
            const uint32_t b = (p >= headBytes && p < headBytes + len) ? line[p - headBytes] : (j & 1 ? 0x7Du : 0x22u);  // junk: '}' and '"'
            q[j >> 2] |= b << ((j & 3) * 8);
        }
    }
    uint32_t stageCount(uint32_t end) const { return (end + kJsonStageBytes - 1) / kJsonStageBytes; }
    void stage(uint32_t s) { stageNow = s; }
    void rowQuad(uint32_t k, uint32_t q[4]) const { quadAt(stageNow * kJsonStageBytes + k * 16, q); }
    uint32_t byteAt(uint32_t p) const { return line[p - headBytes]; }
};

// one line on the host, the DEEP second walk included (what lc_json_walk_host does with two launches)
inline void jsonWalkLineHost(const uint8_t* line, uint32_t len, uint32_t head, uint32_t W, lc_json_member_t* row, uint8_t* shadow,
                             uint8_t* status, uint32_t* nmembers, uint32_t* errpos, bool* wentDeep = nullptr) {
    JsonHostSource src(line, len, head);
    jsonWalkLine<false>(src, len, W, row, shadow, nullptr, status, nmembers, errpos);
    if (wentDeep) *wentDeep = *status == LC_JSON_DEEP;
    if (*status == LC_JSON_DEEP) {
        uint32_t deep[kJsonDeepWords];
        JsonHostSource again(line, len, head);
        jsonWalkLine<true>(again, len, W, row, shadow, deep, status, nmembers, errpos);
    }
}
