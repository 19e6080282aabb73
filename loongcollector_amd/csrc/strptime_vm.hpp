// strptime_vm.hpp -- the per-value routine of processor_parse_timestamp_gpu: ONE template, compiled for the device (strptime_kernel.hpp:
// one value per lane) and for the host (tests/native/timestamp_double.cpp; the processor's %f tail).  It runs a compiled SourceFormat
// (strptime_program.hpp) over one byte span the way the reference's strptime_ns (core/common/Strptime.cpp) runs the format string over
// a NUL-terminated buffer: the end of the span acts as the NUL and nothing behind it is read.  No struct tm, no libc: the broken-down
// fields live in registers and are normalised by calendar arithmetic into civil seconds (the fields read as UTC).
//
// A program is LINEAR: no op jumps.  A value that fails only stops executing, so the program counter is the same for every lane of a
// wavefront and the fetch of an op is a uniform (broadcast) read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_TS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_TS_HD inline
#endif

// ---- status byte of a value (include/lc_timestamp.h repeats these for C callers)
#define LC_TS_OK 0x01u        // the format matched
#define LC_TS_HAS_YEAR 0x02u  // the format delivered a year: secs holds civil seconds.  Clear: secs holds (mon << 40 | mday << 32 | second of day)
#define LC_TS_DST 0x04u       // tm_isdst = 1 was left behind (%z with EDT / CDT / MDT / PDT)
#define LC_TS_EPOCH 0x08u     // the "%s" format: secs is the epoch second itself, no zone applies
#define LC_TS_ABSENT 0x80u    // the capture-table entry: the line did not match, or the group did not take part

// ---- program words: op | llim << 6 | field << 8 | ulim << 16
enum StrptimeOp : uint32_t {
    TS_OP_FAIL = 0,      // an unknown conversion, or a modifier the conversion does not allow (LEGAL_ALT)
    TS_OP_LIT = 1,       // field = the byte
    TS_OP_SPACE = 2,     // any run of white space, also none
    TS_OP_NUM = 3,       // conv_num(llim, ulim) into `field`
    TS_OP_NAME = 4,      // find_string: field = TS_NAME_*
    TS_OP_FRAC = 5,      // %f
    TS_OP_SKIP_G = 6,    // %G: one byte, then every digit
    TS_OP_ZNAME = 7,     // %Z
    TS_OP_ZOFF = 8,      // %z
    TS_OP_EPOCH = 9,     // the whole format is "%s"
    TS_OP_RESET_NS = 10, // entry of a composite conversion (the recursive call clears the nanoseconds)
};
enum StrptimeField : uint32_t {
    TS_F_SEC = 0, TS_F_MIN, TS_F_HOUR, TS_F_MDAY, TS_F_MON1, TS_F_HOUR12, TS_F_YEAR4, TS_F_IGNORE,
    TS_F_CENT_FIRST, TS_F_CENT_SPLIT, TS_F_YY_FIRST, TS_F_YY_SPLIT,
};
enum StrptimeNameTable : uint32_t { TS_NAME_DAY = 0, TS_NAME_MON = 1, TS_NAME_AMPM = 2 };

constexpr uint32_t kStrptimeMaxOps = 64;  // the kernel's program window (LDS)
struct StrptimeProgram {
    uint32_t n;
    uint32_t words[kStrptimeMaxOps];
};
inline constexpr uint32_t tsWord(uint32_t op, uint32_t field = 0, uint32_t llim = 0, uint32_t ulim = 0) {
    return op | (llim << 6) | (field << 8) | (ulim << 16);
}

// ---- the name tables (C locale), upper case, fixed 10-byte entries: [length][bytes].  Long forms before short ones, as find_string
// tries them.  The kernel copies the block into LDS once per workgroup.
constexpr uint32_t kTsNameStride = 10;
constexpr uint32_t kTsDayAt = 0, kTsMonAt = 14, kTsAmPmAt = 38, kTsNastAt = 40, kTsNadtAt = 44, kTsNameCount = 48;
constexpr uint32_t kTsNameBytes = kTsNameCount * kTsNameStride;
struct StrptimeNames {
    uint8_t b[kTsNameBytes];
};
namespace lcts_detail {
constexpr const char* kNames[kTsNameCount] = {
    "SUNDAY", "MONDAY", "TUESDAY", "WEDNESDAY", "THURSDAY", "FRIDAY", "SATURDAY", "SUN", "MON", "TUE", "WED", "THU", "FRI", "SAT",
    "JANUARY", "FEBRUARY", "MARCH", "APRIL", "MAY", "JUNE", "JULY", "AUGUST", "SEPTEMBER", "OCTOBER", "NOVEMBER", "DECEMBER",
    "JAN", "FEB", "MAR", "APR", "MAY", "JUN", "JUL", "AUG", "SEP", "OCT", "NOV", "DEC",
    "AM", "PM", "EST", "CST", "MST", "PST", "EDT", "CDT", "MDT", "PDT"};
constexpr StrptimeNames makeNames() {
    StrptimeNames t{};
    for (uint32_t i = 0; i < kTsNameCount; ++i) {
        uint32_t l = 0;
        while (kNames[i][l]) {
            t.b[i * kTsNameStride + 1 + l] = uint8_t(kNames[i][l]);
            ++l;
        }
        t.b[i * kTsNameStride] = uint8_t(l);
    }
    return t;
}
}  // namespace lcts_detail
constexpr StrptimeNames kStrptimeNames = lcts_detail::makeNames();

// what a value comes to
struct StrptimeResult {
    uint8_t status;
    int64_t secs;
    uint32_t nanos;    // the reference's unsigned 32-bit accumulator: beyond nine digits it wraps, as conv_nanosecond's does
    int32_t matched;   // bytes the format consumed (strptime_ns's return value minus the buffer); 0 on failure
    int32_t fracLen;   // digits %f (or the tail of %s) consumed; 0: none
};

LC_TS_HD bool tsIsSpace(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }
LC_TS_HD bool tsIsDigit(uint32_t c) { return c - '0' < 10u; }
LC_TS_HD uint32_t tsUpper(uint32_t c) { return (c - 'a' < 26u) ? c - 32 : c; }

// days from 1970-01-01 to y-01-01 (proleptic Gregorian; y may be any int32 year)
LC_TS_HD int64_t tsDaysToYear(int64_t y) {
    const int64_t p = y - 1;  // floor divisions, p may be negative
    const int64_t d4 = p >= 0 ? p / 4 : -((-p + 3) / 4);
    const int64_t d100 = p >= 0 ? p / 100 : -((-p + 99) / 100);
    const int64_t d400 = p >= 0 ? p / 400 : -((-p + 399) / 400);
    return 365 * (y - 1970) + (d4 - 492) - (d100 - 19) + (d400 - 4);
}
LC_TS_HD bool tsIsLeap(int64_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
LC_TS_HD uint32_t tsDaysBeforeMonth(uint32_t mon, bool leap) {  // mon 0..11
    // cumulative days of a non-leap year; a select chain, so that no table in memory is read
    const uint32_t cum = mon == 0 ? 0 : mon == 1 ? 31 : mon == 2 ? 59 : mon == 3 ? 90 : mon == 4 ? 120 : mon == 5 ? 151 : mon == 6 ? 181
                       : mon == 7 ? 212 : mon == 8 ? 243 : mon == 9 ? 273 : mon == 10 ? 304 : 334;
    return cum + ((leap && mon >= 2) ? 1u : 0u);
}
// civil seconds of (year, mon 0..11, any mday, second of day): what timegm / mktime-under-UTC make of the fields
LC_TS_HD int64_t tsCivilSeconds(int64_t year, uint32_t mon, int32_t mday, int64_t tod) {
    const int64_t days = tsDaysToYear(year) + int64_t(tsDaysBeforeMonth(mon, tsIsLeap(year))) + (int64_t(mday) - 1);
    return days * 86400 + tod;
}

// conv_nanosecond at `pos`: false when no digit stands there
template <class Source>
LC_TS_HD bool tsConvNanos(const Source& src, uint32_t len, uint32_t& pos, uint32_t& nanos, int32_t& fracLen) {
    uint32_t ch = pos < len ? src.at(pos) : 0u;
    if (!tsIsDigit(ch)) return false;
    uint32_t result = 0, digits = 0;
    do {
        result = result * 10u + (ch - '0');
        ++digits;
        ++pos;
        ch = pos < len ? src.at(pos) : 0u;
    } while (tsIsDigit(ch));
    for (uint32_t i = digits; i < 9; ++i) result *= 10u;
    nanos = result;
    fracLen = int32_t(digits);
    return true;
}

// conv_num(llim, ulim) at `pos`: false when no digit stands there (pos stays) or the number is out of range (pos is behind the digits
// it took); v is written on success only
template <class Source>
LC_TS_HD bool tsConvNum(const Source& src, uint32_t len, uint32_t& pos, uint32_t llim, uint32_t ulim, int32_t& v) {
    uint32_t ch = pos < len ? src.at(pos) : 0u;
    if (!tsIsDigit(ch)) return false;
    uint32_t result = 0, rulim = ulim;
    do {
        result = result * 10u + (ch - '0');
        rulim /= 10u;
        ++pos;
        ch = pos < len ? src.at(pos) : 0u;
    } while (result * 10u <= ulim && rulim && tsIsDigit(ch));
    if (result < llim || result > ulim) return false;
    v = int32_t(result);
    return true;
}

// the "%s" format over the whole span.  strtoll: white space, one sign, digits (saturating); then the reference keeps the first ten
// characters of the decimal rendering as the second and reads what follows the tenth byte OF THE BUFFER as the fraction.  false: no
// digit, or a second of 0.  pos: behind the digits strtoll took
template <class Source>
LC_TS_HD bool tsConvEpoch(const Source& src, uint32_t len, int64_t& epochSecs, uint32_t& nanos, int32_t& fracLen, uint32_t& pos) {
    uint32_t p = 0;
    while (p < len && tsIsSpace(src.at(p))) ++p;
    bool neg = false;
    if (p < len && (src.at(p) == '+' || src.at(p) == '-')) {
        neg = src.at(p) == '-';
        ++p;
    }
    uint64_t mag = 0;
    const uint64_t lim = neg ? 9223372036854775808ull : 9223372036854775807ull;
    uint32_t nd = 0;
    bool sat = false;
    while (p < len && tsIsDigit(src.at(p))) {
        const uint32_t d = src.at(p) - '0';
        if (sat || mag > (lim - d) / 10) {
            sat = true;
            mag = lim;
        } else {
            mag = mag * 10 + d;
        }
        ++p;
        ++nd;
    }
    uint32_t rendered = neg && mag ? 1u : 0u;  // std::to_string(n).length()
    {
        uint64_t t = mag;
        do {
            ++rendered;
            t /= 10;
        } while (t);
    }
    const uint32_t keep = rendered >= 10 ? 10u : rendered;
    for (uint32_t i = keep; i < rendered; ++i) mag /= 10;  // (truncation toward zero, the sign aside)
    if (nd == 0 || mag == 0) return false;
    epochSecs = neg ? -int64_t(mag) : int64_t(mag);
    uint32_t q = keep;
    (void)tsConvNanos(src, len, q, nanos, fracLen);
    pos = p;
    return true;
}

// Source: uint32_t at(uint32_t i) const for i < len.  prog / names: pointers (of any address space: LDS on the device) to the program
// words and to the name block.  The routine never calls at() with i >= len.
template <class Source, class ProgPtr, class NamePtr>
LC_TS_HD StrptimeResult strptimeRun(const Source& src, uint32_t len, ProgPtr prog, uint32_t nOps, NamePtr names) {
    constexpr int32_t kNoYear = INT32_MIN;
    int32_t sec = 0, min = 0, hour = 0, mday = 0, mon = 0, year = kNoYear;
    uint32_t dst = 0, nanos = 0, pos = 0, epoch = 0;
    int32_t fracLen = 0;
    int64_t epochSecs = 0;
    bool fail = false;
#define TS_AT(i) ((i) < len ? src.at(i) : 0u)
    for (uint32_t pc = 0; pc < nOps; ++pc) {
        const uint32_t w = prog[pc];  // (uniform over the wavefront: pc does not depend on the value)
        if (fail) {
#if defined(__HIP_DEVICE_COMPILE__)
            continue;
#else
            break;
#endif
        }
        const uint32_t op = w & 63u, field = (w >> 8) & 255u;
        switch (op) {
            case TS_OP_LIT:
                if (TS_AT(pos) != field) fail = true;
                ++pos;  // (a failed value's position is never read again)
                break;
            case TS_OP_SPACE:
                while (pos < len && tsIsSpace(src.at(pos))) ++pos;
                break;
            case TS_OP_NUM: {
                const uint32_t llim = (w >> 6) & 1u, ulim = w >> 16;
                // the value the reference's variable holds when conv_num leaves it alone
                int32_t v = 0;
                switch (field) {
                    case TS_F_SEC: v = sec; break;
                    case TS_F_MIN: v = min; break;
                    case TS_F_HOUR: case TS_F_HOUR12: v = hour; break;
                    case TS_F_MDAY: v = mday; break;
                    case TS_F_MON1: v = 1; break;
                    case TS_F_YEAR4: v = 1900; break;
                    case TS_F_CENT_FIRST: case TS_F_CENT_SPLIT: v = 20; break;
                    default: v = 0; break;
                }
                if (!tsConvNum(src, len, pos, llim, ulim, v)) fail = true;
                // the statements behind conv_num run whether or not it succeeded
                switch (field) {
                    case TS_F_SEC: sec = v; break;
                    case TS_F_MIN: min = v; break;
                    case TS_F_HOUR: hour = v; break;
                    case TS_F_HOUR12: hour = v == 12 ? 0 : v; break;
                    case TS_F_MDAY: mday = v; break;
                    case TS_F_MON1: mon = v - 1; break;
                    case TS_F_YEAR4: year = v - 1900; break;
                    case TS_F_CENT_FIRST: year = v * 100 - 1900; break;
                    case TS_F_CENT_SPLIT: year = v * 100 - 1900 + year % 100; break;
                    case TS_F_YY_FIRST: year = v <= 68 ? v + 100 : v; break;
                    case TS_F_YY_SPLIT: year = v + (year / 100) * 100; break;
                    default: break;
                }
                break;
            }
            case TS_OP_NAME: {
                const uint32_t first = field == TS_NAME_DAY ? kTsDayAt : field == TS_NAME_MON ? kTsMonAt : kTsAmPmAt;
                const uint32_t count = field == TS_NAME_DAY ? 14u : field == TS_NAME_MON ? 24u : 2u;
                const uint32_t half = field == TS_NAME_DAY ? 7u : field == TS_NAME_MON ? 12u : 2u;
                int32_t found = -1;
                uint32_t foundLen = 0;
                for (uint32_t k = 0; k < count && found < 0; ++k) {
                    const NamePtr e = names + (first + k) * kTsNameStride;
                    const uint32_t l = e[0];
                    bool eq = pos + l <= len;
                    for (uint32_t j = 0; eq && j < l; ++j) eq = tsUpper(src.at(pos + j)) == e[1 + j];
                    if (eq) {
                        found = int32_t(k % half);
                        foundLen = l;
                    }
                }
                if (found < 0) fail = true;
                else pos += foundLen;
                if (field == TS_NAME_MON) {
                    if (found >= 0) mon = found;
                } else if (field == TS_NAME_AMPM) {
                    if (hour > 11) fail = true;
                    else if (found > 0) hour += 12;
                }
                break;
            }
            case TS_OP_FRAC:
                if (!tsConvNanos(src, len, pos, nanos, fracLen)) fail = true;
                break;
            case TS_OP_SKIP_G:
                // the reference steps over one byte unseen, the NUL included; the span's end is where this routine stops instead
                if (pos >= len) {
                    fail = true;
                } else {
                    do ++pos;
                    while (pos < len && tsIsDigit(src.at(pos)));
                }
                break;
            case TS_OP_ZNAME:
                if (pos + 3 <= len) {
                    const uint32_t a = tsUpper(src.at(pos)), b = tsUpper(src.at(pos + 1)), c = tsUpper(src.at(pos + 2));
                    if ((a == 'G' && b == 'M' && c == 'T') || (a == 'U' && b == 'T' && c == 'C')) {
                        dst = 0;
                        pos += 3;
                    }
                }
                break;
            case TS_OP_ZOFF: {
                while (pos < len && tsIsSpace(src.at(pos))) ++pos;
                uint32_t c = TS_AT(pos);
                ++pos;
                bool numeric = false;
                if (c == 'G' || c == 'U' || c == 'Z') {
                    if (c == 'G') {
                        if (TS_AT(pos) != 'M') fail = true;
                        ++pos;
                    }
                    if (!fail && c != 'Z') {
                        if (TS_AT(pos) != 'T') fail = true;
                        ++pos;
                    }
                    if (!fail) dst = 0;
                } else if (c == '+' || c == '-') {
                    numeric = true;
                } else {
                    --pos;
                    int32_t found = -1;  // EST CST MST PST, then EDT CDT MDT PDT
                    for (uint32_t k = 0; k < 8 && found < 0; ++k) {
                        const NamePtr e = names + (kTsNastAt + k) * kTsNameStride;
                        bool eq = pos + 3 <= len;
                        for (uint32_t j = 0; eq && j < 3; ++j) eq = tsUpper(src.at(pos + j)) == e[1 + j];
                        if (eq) found = int32_t(k);
                    }
                    if (found >= 0) {
                        pos += 3;
                        if (found >= 4) dst = 1;
                    } else if ((c >= 'A' && c <= 'I') || (c >= 'L' && c <= 'Y')) {
                        ++pos;  // a military zone letter
                    } else {
                        fail = true;
                    }
                }
                if (numeric) {
                    uint32_t offs = 0, i = 0;
                    while (i < 4) {
                        const uint32_t d = TS_AT(pos);
                        if (tsIsDigit(d)) {
                            offs = offs * 10 + (d - '0');
                            ++pos;
                            ++i;
                            continue;
                        }
                        if (i == 2 && d == ':') {
                            ++pos;
                            continue;
                        }
                        break;
                    }
                    if (i == 4) {
                        if (offs % 100 >= 60) fail = true;
                    } else if (i != 2) {
                        fail = true;
                    }
                    if (!fail) dst = 0;
                }
                break;
            }
            case TS_OP_EPOCH:
                if (tsConvEpoch(src, len, epochSecs, nanos, fracLen, pos)) epoch = 1;
                else fail = true;
                break;
            case TS_OP_RESET_NS:
                nanos = 0;
                break;
            default:  // TS_OP_FAIL
                fail = true;
                break;
        }
    }
#undef TS_AT
    StrptimeResult r;
    r.nanos = nanos;
    r.fracLen = fail ? 0 : fracLen;
    r.matched = fail ? 0 : int32_t(pos);
    uint32_t st = fail ? 0u : LC_TS_OK;
    if (dst) st |= LC_TS_DST;
    const int64_t tod = int64_t(hour) * 3600 + int64_t(min) * 60 + int64_t(sec);
    if (epoch) {
        st |= LC_TS_EPOCH | LC_TS_HAS_YEAR;
        r.secs = epochSecs;
    } else if (year != kNoYear) {
        st |= LC_TS_HAS_YEAR;
        r.secs = tsCivilSeconds(int64_t(year) + 1900, uint32_t(mon), mday, tod);
    } else {
        r.secs = (int64_t(mon) << 40) | (int64_t(mday) << 32) | tod;
    }
    r.status = uint8_t(st);
    return r;
}

// the host's view of one value (the CPU double, the tools)
struct HostSpanSource {
    const uint8_t* p;
    uint32_t at(uint32_t i) const { return p[i]; }
};
