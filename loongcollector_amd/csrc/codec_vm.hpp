// codec_vm.hpp -- the per-unit routines of the field codecs (include/codec/lc_codec.h), written ONCE for the host and the device: the
// base64 classifier and the decode state that crosses 16-byte units, the 12 -> 16 and 16 -> 12 conversions on whole words, MD5 padding
// and the lower-case hex writer (md5Block itself is desens_vm.hpp's).  codec_kernel.hpp runs them per lane; the host routines at the
// end walk one value with them the way the kernels do, for tests/native/codec_host_check.cpp and tests/native/codec_double.cpp.
// Words are little-endian: byte i of a unit is bits [8 * (i % 4), +8) of word i / 4.
#pragma once

#include <cstdint>
#include <cstring>

#include "desens_vm.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_CODEC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_CODEC_HD inline
#endif

constexpr uint32_t kCodecEncode = 0, kCodecDecode = 1, kCodecMd5 = 2;
constexpr uint8_t kCodecFlagOut = 1, kCodecFlagError = 2;  // LC_CODEC_OUT, LC_CODEC_ERROR

struct CodecConfig {
    uint32_t op = kCodecEncode;
};

// ---------------------------------------------------------------------------------------------- the alphabet
// a byte's class: its sextet (0..63), or one of these
constexpr uint32_t kB64Other = 64, kB64Skip = 65, kB64Pad = 66;

LC_CODEC_HD uint32_t b64Class(uint32_t c) {
    uint32_t r = kB64Other;
    r = c - 'A' < 26u ? c - 'A' : r;
    r = c - 'a' < 26u ? c - 'a' + 26u : r;
    r = c - '0' < 10u ? c - '0' + 52u : r;
    r = c == '+' ? 62u : r;
    r = c == '/' ? 63u : r;
    r = c == '=' ? kB64Pad : r;
    r = (c == '\r' || c == '\n') ? kB64Skip : r;
    return r;
}
LC_CODEC_HD uint32_t b64Char(uint32_t s) {
    return s + 65u + (s >= 26u ? 6u : 0u) - (s >= 52u ? 75u : 0u) - (s >= 62u ? 15u : 0u) + (s >= 63u ? 3u : 0u);
}
LC_CODEC_HD uint32_t codecEncodedLen(uint32_t len) { return 4u * ((len + 2u) / 3u); }
LC_CODEC_HD uint32_t codecRound16(uint32_t len) { return (len + 15u) & ~15u; }

// ---------------------------------------------------------------------------------------------- encode: 12 bytes -> 16 characters
// t: three bytes, the first in the low bits -> four characters, the first in the low bits
LC_CODEC_HD uint32_t b64Encode3(uint32_t t) {
    const uint32_t b0 = t & 255u, b1 = (t >> 8) & 255u, b2 = (t >> 16) & 255u;
    return b64Char(b0 >> 2) | b64Char(((b0 & 3u) << 4) | (b1 >> 4)) << 8 | b64Char(((b1 & 15u) << 2) | (b2 >> 6)) << 16 | b64Char(b2 & 63u) << 24;
}
LC_CODEC_HD void b64Encode12(const uint32_t w[3], uint32_t out[4]) {
    out[0] = b64Encode3(w[0] & 0xFFFFFFu);
    out[1] = b64Encode3((w[0] >> 24) | ((w[1] & 0xFFFFu) << 8));
    out[2] = b64Encode3((w[1] >> 16) | ((w[2] & 0xFFu) << 16));
    out[3] = b64Encode3(w[2] >> 8);
}
// the last unit of a value: r bytes (1..11) of w count, whatever stands behind them -> the number of words of out that are written
LC_CODEC_HD uint32_t b64EncodeTail(const uint32_t w[3], uint32_t r, uint32_t out[4]) {
    uint32_t m[3];
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i) {
        const uint32_t keep = r > 4 * i ? (r - 4 * i < 4u ? r - 4 * i : 4u) : 0u;
        m[i] = keep == 4 ? w[i] : keep ? w[i] & ((1u << (8 * keep)) - 1u) : 0u;
    }
    b64Encode12(m, out);
    const uint32_t groups = (r + 2) / 3, rem = r % 3;
    if (rem) {
        const uint32_t pad = rem == 1 ? 0x3D3D0000u : 0x3D000000u, keepMask = rem == 1 ? 0x0000FFFFu : 0x00FFFFFFu;
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g)
            if (g == groups - 1) out[g] = (out[g] & keepMask) | pad;
    }
    return groups;
}

// ---------------------------------------------------------------------------------------------- decode: the size pass
// what crosses a unit border.  phase: 0 in the quanta, 1 behind the first `=` of two, 2 behind the padding
struct B64DecodeState {
    uint32_t k = 0, phase = 0, err = 0, errOff = 0, sawSkip = 0;
};
// the byte c at raw position p of the value
LC_CODEC_HD void b64DecodeByte(B64DecodeState& s, uint32_t c, uint32_t p) {
    const uint32_t cls = b64Class(c);
    if (cls == kB64Skip) {
        s.sawSkip = 1;
        return;
    }
    if (s.err) return;  // the first error wins
    if (s.phase == 0) {
        if (cls < 64u) {
            ++s.k;
        } else if (cls == kB64Pad && (s.k & 3u) >= 2u) {
            s.phase = (s.k & 3u) == 2u ? 1u : 2u;
        } else {
            s.err = 1;
            s.errOff = p;
        }
    } else if (s.phase == 1 && cls == kB64Pad) {
        s.phase = 2;
    } else {
        s.err = 1;
        s.errOff = s.phase == 1 ? p - 1 : p;  // (Go's quirk behind a single `=`)
    }
}
// the bytes [from, to) of the unit q (0 <= from <= to <= 16); unitPos: the raw position of the unit's byte 0 (may be "negative": only
// from.. count)
LC_CODEC_HD void b64DecodeUnit(B64DecodeState& s, const uint32_t q[4], uint32_t from, uint32_t to, uint32_t unitPos) {
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (i >= from && i < to) b64DecodeByte(s, (q[i >> 2] >> (8 * (i & 3u))) & 255u, unitPos + i);
}
// the value's end -> its flags; *outLen (0 on an error), *errOff (on an error)
LC_CODEC_HD uint32_t b64DecodeFinish(const B64DecodeState& s, uint32_t len, uint32_t* outLen, uint32_t* errOff) {
    *outLen = 0;
    *errOff = 0;
    const uint32_t j = s.k & 3u;
    if (s.err) {
        *errOff = s.errOff;
        return kCodecFlagError;
    }
    if (s.phase == 1 || (s.phase == 0 && j != 0)) {
        *errOff = s.phase == 1 ? len : len - j;
        return kCodecFlagError;
    }
    *outLen = 3u * (s.k >> 2) + (s.phase == 2 ? j - 1u : 0u);
    return kCodecFlagOut;
}
// the number of sextets behind outLen decoded bytes
LC_CODEC_HD uint32_t b64SextetsOf(uint32_t outLen) { return (outLen / 3u) * 4u + (outLen % 3u ? outLen % 3u + 1u : 0u); }

// ---------------------------------------------------------------------------------------------- decode: 16 characters -> 12 bytes
// four characters -> their four sextets, one per byte (a byte that is no alphabet byte gives bits nobody stores)
LC_CODEC_HD uint32_t b64Sextets4(uint32_t chars) {
    return (b64Class(chars & 255u) & 63u) | (b64Class((chars >> 8) & 255u) & 63u) << 8 | (b64Class((chars >> 16) & 255u) & 63u) << 16 |
           (b64Class(chars >> 24) & 63u) << 24;
}
// four sextets, one per byte -> three bytes, the first in the low bits
LC_CODEC_HD uint32_t b64Decode4(uint32_t s) {
    const uint32_t a = s & 63u, b = (s >> 8) & 63u, c = (s >> 16) & 63u, d = (s >> 24) & 63u;
    return ((a << 2) | (b >> 4)) | (((b & 15u) << 4) | (c >> 2)) << 8 | (((c & 3u) << 6) | d) << 16;
}
LC_CODEC_HD void b64Decode16(const uint32_t s[4], uint32_t out[3]) {
    const uint32_t t0 = b64Decode4(s[0]), t1 = b64Decode4(s[1]), t2 = b64Decode4(s[2]), t3 = b64Decode4(s[3]);
    out[0] = t0 | t1 << 24;
    out[1] = t1 >> 8 | t2 << 16;
    out[2] = t2 >> 16 | t3 << 8;
}
// the bytes a unit of m sextets (1..16) gives
LC_CODEC_HD uint32_t b64UnitBytes(uint32_t m) { return (m * 3u) >> 2; }

// ---------------------------------------------------------------------------------------------- MD5
LC_CODEC_HD uint32_t md5Blocks(uint32_t len) { return (len + 8u) / 64u + 1u; }
// x: the message's word at byte offset q, whatever stands behind the message's end -> the padded message's word (without the length)
LC_CODEC_HD uint32_t md5PaddedWord(uint32_t x, uint32_t q, uint32_t len) {
    if (q + 4u <= len) return x;
    if (q > len) return 0u;
    const uint32_t r = len - q;  // 0..3 bytes of the message
    return (r ? x & ((1u << (8 * r)) - 1u) : 0u) | 0x80u << (8 * r);
}
LC_CODEC_HD uint32_t hexLower(uint32_t n) { return n + 48u + (n > 9u ? 39u : 0u); }
// the state -> 32 lower-case hex digits as eight words
LC_CODEC_HD void md5HexLower(const uint32_t h[4], uint32_t out[8]) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t w = h[i];
        out[2 * i] = hexLower((w >> 4) & 15u) | hexLower(w & 15u) << 8 | hexLower((w >> 12) & 15u) << 16 | hexLower((w >> 8) & 15u) << 24;
        out[2 * i + 1] = hexLower((w >> 20) & 15u) | hexLower((w >> 16) & 15u) << 8 | hexLower(w >> 28) << 16 | hexLower((w >> 24) & 15u) << 24;
    }
}
LC_CODEC_HD void md5Init(uint32_t h[4]) {
    h[0] = 0x67452301u;
    h[1] = 0xefcdab89u;
    h[2] = 0x98badcfeu;
    h[3] = 0x10325476u;
}
// block j of the padded message from its sixteen raw words
LC_CODEC_HD void md5PadBlock(uint32_t x[16], uint32_t j, uint32_t len) {
#pragma unroll
    for (uint32_t d = 0; d < 16; ++d) x[d] = md5PaddedWord(x[d], 64u * j + 4u * d, len);
    if (j == md5Blocks(len) - 1u) {
        x[14] = len << 3;
        x[15] = len >> 29;
    }
}

// ---------------------------------------------------------------------------------------------- one value on the host
#if !defined(__HIP_DEVICE_COMPILE__)
namespace codechost {
constexpr uint8_t kBehind = 0xEE;  // what the host routines put where a kernel's word load reads behind the value
inline uint32_t wordAt(const uint8_t* v, uint32_t len, uint32_t at) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b) w |= uint32_t(at + b < len ? v[at + b] : kBehind) << (8 * b);
    return w;
}
inline void putWord(uint8_t* out, uint32_t w) { std::memcpy(out, &w, 4); }
}  // namespace codechost

// out: codecEncodedLen(len) bytes
inline void codecEncodeHost(const uint8_t* v, uint32_t len, uint8_t* out) {
    for (uint32_t u = 0; u * 12 < len; ++u) {
        const uint32_t w[3] = {codechost::wordAt(v, len, 12 * u), codechost::wordAt(v, len, 12 * u + 4), codechost::wordAt(v, len, 12 * u + 8)};
        uint32_t o[4];
        const uint32_t r = len - 12 * u;
        const uint32_t words = r >= 12 ? (b64Encode12(w, o), 4u) : b64EncodeTail(w, r, o);
        for (uint32_t g = 0; g < words; ++g) codechost::putWord(out + 16 * u + 4 * g, o[g]);
    }
}
// the size pass in 16-byte units counted from the 16-byte boundary `head` bytes in front of the value -> flags
inline uint32_t codecDecodeSizeHost(const uint8_t* v, uint32_t len, uint32_t head, uint32_t* outLen, uint32_t* errOff, bool* clean) {
    B64DecodeState s;
    const uint32_t end = head + len;
    for (uint32_t ub = 0; ub < end; ub += 16) {
        const uint32_t from = ub < head ? head - ub : 0u, to = end - ub < 16u ? end - ub : 16u;
        uint32_t q[4];
        for (uint32_t i = 0; i < 4; ++i) {
            q[i] = 0;
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t p = ub + 4 * i + b;
                q[i] |= uint32_t(p >= head && p < end ? v[p - head] : codechost::kBehind) << (8 * b);
            }
        }
        b64DecodeUnit(s, q, from, to, ub - head);
    }
    *clean = !s.sawSkip;
    return b64DecodeFinish(s, len, outLen, errOff);
}
// the write pass of a value the size pass accepted; out: outLen bytes
inline void codecDecodeWriteHost(const uint8_t* v, uint32_t len, bool clean, uint32_t outLen, uint8_t* out) {
    const uint32_t sextets = b64SextetsOf(outLen);
    auto unit = [&](uint32_t u, const uint32_t s[4]) {
        const uint32_t m = sextets - 16 * u < 16u ? sextets - 16 * u : 16u, bytes = b64UnitBytes(m);
        uint32_t o[3];
        b64Decode16(s, o);
        for (uint32_t g = 0; g < 3; ++g) {
            if (4 * g + 4 <= bytes) codechost::putWord(out + 12 * u + 4 * g, o[g]);
            else
                for (uint32_t b = 4 * g; b < bytes; ++b) out[12 * u + b] = uint8_t(o[g] >> (8 * (b & 3u)));
        }
    };
    if (clean) {
        for (uint32_t u = 0; 16 * u < sextets; ++u) {
            uint32_t s[4];
            for (uint32_t i = 0; i < 4; ++i) s[i] = b64Sextets4(codechost::wordAt(v, len, 16 * u + 4 * i));
            unit(u, s);
        }
        return;
    }
    // with CR/LF: the significant characters compacted by rank, sixteen sextets staged per unit
    uint8_t staged[16];
    uint32_t rank = 0;
    auto flush = [&](uint32_t u) {
        uint32_t s[4];
        std::memcpy(s, staged, 16);
        unit(u, s);
    };
    for (uint32_t p = 0; p < len && rank < sextets; ++p) {
        const uint32_t cls = b64Class(v[p]);
        if (cls >= 64u) continue;
        staged[rank & 15u] = uint8_t(cls);
        if ((++rank & 15u) == 0) flush(rank / 16 - 1);
    }
    if (rank & 15u) {
        std::memset(staged + (rank & 15u), 0, 16 - (rank & 15u));
        flush(rank / 16);
    }
}
// out: 32 bytes
inline void codecMd5Host(const uint8_t* v, uint32_t len, uint8_t* out) {
    uint32_t h[4];
    md5Init(h);
    for (uint32_t j = 0; j < md5Blocks(len); ++j) {
        uint32_t x[16];
        for (uint32_t d = 0; d < 16; ++d) x[d] = codechost::wordAt(v, len, 64 * j + 4 * d);
        md5PadBlock(x, j, len);
        lcdesens::md5Block(h, x);
    }
    uint32_t o[8];
    md5HexLower(h, o);
    for (uint32_t g = 0; g < 8; ++g) codechost::putWord(out + 4 * g, o[g]);
}
#endif
