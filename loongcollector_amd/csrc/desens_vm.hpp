// desens_vm.hpp -- the per-value routines of processor_desensitize_gpu (include/lc_desensitize.h), written ONCE for the host and the
// device: the MD5 of a byte range as 32 upper-case hex digits, the rule that turns one search result into a cut (the two disciplines of
// ProcessorDesensitizeNative::CastOneSensitiveWord, core/plugin/processor/ProcessorDesensitizeNative.cpp:198-249), the output length of
// a value from its cut list, and the writer that lays `prefix | rewrite pieces or digest | ... | tail` into an output range.  The
// kernels of desens_kernel.hpp call these with (lane, 64); the host walk (desensWalkValue, tests/native/desens_host_check.cpp) with (0, 1).
//
// A value's cuts are a chain of RECORDS, newest first: words [prev, cutB, me, (b, e) per referenced group].
//   const: [cutB, me) is the whole match and is replaced by the rewrite program's pieces (literal bytes and group spans);
//   md5:   cutB is where the `before` group ends; [cutB, me) is replaced by MD5(value[cutB:me)).
// The bytes between two cuts, in front of the first and behind the last are the value's own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC_DESENS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_DESENS_HD inline
#endif

namespace lcdesens {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMethodConst = 0, kMethodMd5 = 1;
constexpr uint32_t kPieceLiteral = 0, kPieceGroup = 1;
constexpr uint32_t kRecHead = 3;  // prev, cutB, me
// per-line status bytes of the match engine (include/lc_regex_gpu.h)
constexpr uint8_t kStatusMatch = 1;
// per-value flags (include/lc_desensitize.h LC_DESENS_*)
constexpr uint8_t kFlagChanged = 1, kFlagGaveUp = 2;

// The parsed rewrite: pieces of three words {kind, a, b} -- literal: a = offset into lit, b = length; group: a = the span's slot in a
// record.  nRef spans ride in every record of a `const` handle, none in an `md5` one.
struct Program {
    uint32_t method = kMethodConst;
    uint32_t nPieces = 0;
    uint32_t nRef = 0;
    const uint32_t* pieces = nullptr;
    const uint8_t* lit = nullptr;
};
LC_DESENS_HD uint32_t recWords(const Program& P) { return kRecHead + 2 * P.nRef; }

// ---------------------------------------------------------------------------------------------- MD5 (RFC 1321)
LC_DESENS_HD uint32_t rotl(uint32_t x, int c) { return (x << c) | (x >> (32 - c)); }
// byte q of the padded message of `len` bytes at p
LC_DESENS_HD uint32_t md5Byte(const uint8_t* p, uint32_t len, uint32_t q) { return q < len ? p[q] : q == len ? 0x80u : 0u; }

#define LC_MD5_STEP(f, a, b, c, d, k, s, t) \
    a += f(b, c, d) + x[k] + t;             \
    a = b + rotl(a, s);
#define LC_MD5_F(b, c, d) ((b & c) | (~b & d))
#define LC_MD5_G(b, c, d) ((b & d) | (c & ~d))
#define LC_MD5_H(b, c, d) (b ^ c ^ d)
#define LC_MD5_I(b, c, d) (c ^ (b | ~d))

LC_DESENS_HD void md5Block(uint32_t h[4], const uint32_t x[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    LC_MD5_STEP(LC_MD5_F, a, b, c, d, 0, 7, 0xd76aa478u) LC_MD5_STEP(LC_MD5_F, d, a, b, c, 1, 12, 0xe8c7b756u)
    LC_MD5_STEP(LC_MD5_F, c, d, a, b, 2, 17, 0x242070dbu) LC_MD5_STEP(LC_MD5_F, b, c, d, a, 3, 22, 0xc1bdceeeu)
    LC_MD5_STEP(LC_MD5_F, a, b, c, d, 4, 7, 0xf57c0fafu) LC_MD5_STEP(LC_MD5_F, d, a, b, c, 5, 12, 0x4787c62au)
    LC_MD5_STEP(LC_MD5_F, c, d, a, b, 6, 17, 0xa8304613u) LC_MD5_STEP(LC_MD5_F, b, c, d, a, 7, 22, 0xfd469501u)
    LC_MD5_STEP(LC_MD5_F, a, b, c, d, 8, 7, 0x698098d8u) LC_MD5_STEP(LC_MD5_F, d, a, b, c, 9, 12, 0x8b44f7afu)
    LC_MD5_STEP(LC_MD5_F, c, d, a, b, 10, 17, 0xffff5bb1u) LC_MD5_STEP(LC_MD5_F, b, c, d, a, 11, 22, 0x895cd7beu)
    LC_MD5_STEP(LC_MD5_F, a, b, c, d, 12, 7, 0x6b901122u) LC_MD5_STEP(LC_MD5_F, d, a, b, c, 13, 12, 0xfd987193u)
    LC_MD5_STEP(LC_MD5_F, c, d, a, b, 14, 17, 0xa679438eu) LC_MD5_STEP(LC_MD5_F, b, c, d, a, 15, 22, 0x49b40821u)
    LC_MD5_STEP(LC_MD5_G, a, b, c, d, 1, 5, 0xf61e2562u) LC_MD5_STEP(LC_MD5_G, d, a, b, c, 6, 9, 0xc040b340u)
    LC_MD5_STEP(LC_MD5_G, c, d, a, b, 11, 14, 0x265e5a51u) LC_MD5_STEP(LC_MD5_G, b, c, d, a, 0, 20, 0xe9b6c7aau)
    LC_MD5_STEP(LC_MD5_G, a, b, c, d, 5, 5, 0xd62f105du) LC_MD5_STEP(LC_MD5_G, d, a, b, c, 10, 9, 0x02441453u)
    LC_MD5_STEP(LC_MD5_G, c, d, a, b, 15, 14, 0xd8a1e681u) LC_MD5_STEP(LC_MD5_G, b, c, d, a, 4, 20, 0xe7d3fbc8u)
    LC_MD5_STEP(LC_MD5_G, a, b, c, d, 9, 5, 0x21e1cde6u) LC_MD5_STEP(LC_MD5_G, d, a, b, c, 14, 9, 0xc33707d6u)
    LC_MD5_STEP(LC_MD5_G, c, d, a, b, 3, 14, 0xf4d50d87u) LC_MD5_STEP(LC_MD5_G, b, c, d, a, 8, 20, 0x455a14edu)
    LC_MD5_STEP(LC_MD5_G, a, b, c, d, 13, 5, 0xa9e3e905u) LC_MD5_STEP(LC_MD5_G, d, a, b, c, 2, 9, 0xfcefa3f8u)
    LC_MD5_STEP(LC_MD5_G, c, d, a, b, 7, 14, 0x676f02d9u) LC_MD5_STEP(LC_MD5_G, b, c, d, a, 12, 20, 0x8d2a4c8au)
    LC_MD5_STEP(LC_MD5_H, a, b, c, d, 5, 4, 0xfffa3942u) LC_MD5_STEP(LC_MD5_H, d, a, b, c, 8, 11, 0x8771f681u)
    LC_MD5_STEP(LC_MD5_H, c, d, a, b, 11, 16, 0x6d9d6122u) LC_MD5_STEP(LC_MD5_H, b, c, d, a, 14, 23, 0xfde5380cu)
    LC_MD5_STEP(LC_MD5_H, a, b, c, d, 1, 4, 0xa4beea44u) LC_MD5_STEP(LC_MD5_H, d, a, b, c, 4, 11, 0x4bdecfa9u)
    LC_MD5_STEP(LC_MD5_H, c, d, a, b, 7, 16, 0xf6bb4b60u) LC_MD5_STEP(LC_MD5_H, b, c, d, a, 10, 23, 0xbebfbc70u)
    LC_MD5_STEP(LC_MD5_H, a, b, c, d, 13, 4, 0x289b7ec6u) LC_MD5_STEP(LC_MD5_H, d, a, b, c, 0, 11, 0xeaa127fau)
    LC_MD5_STEP(LC_MD5_H, c, d, a, b, 3, 16, 0xd4ef3085u) LC_MD5_STEP(LC_MD5_H, b, c, d, a, 6, 23, 0x04881d05u)
    LC_MD5_STEP(LC_MD5_H, a, b, c, d, 9, 4, 0xd9d4d039u) LC_MD5_STEP(LC_MD5_H, d, a, b, c, 12, 11, 0xe6db99e5u)
    LC_MD5_STEP(LC_MD5_H, c, d, a, b, 15, 16, 0x1fa27cf8u) LC_MD5_STEP(LC_MD5_H, b, c, d, a, 2, 23, 0xc4ac5665u)
    LC_MD5_STEP(LC_MD5_I, a, b, c, d, 0, 6, 0xf4292244u) LC_MD5_STEP(LC_MD5_I, d, a, b, c, 7, 10, 0x432aff97u)
    LC_MD5_STEP(LC_MD5_I, c, d, a, b, 14, 15, 0xab9423a7u) LC_MD5_STEP(LC_MD5_I, b, c, d, a, 5, 21, 0xfc93a039u)
    LC_MD5_STEP(LC_MD5_I, a, b, c, d, 12, 6, 0x655b59c3u) LC_MD5_STEP(LC_MD5_I, d, a, b, c, 3, 10, 0x8f0ccc92u)
    LC_MD5_STEP(LC_MD5_I, c, d, a, b, 10, 15, 0xffeff47du) LC_MD5_STEP(LC_MD5_I, b, c, d, a, 1, 21, 0x85845dd1u)
    LC_MD5_STEP(LC_MD5_I, a, b, c, d, 8, 6, 0x6fa87e4fu) LC_MD5_STEP(LC_MD5_I, d, a, b, c, 15, 10, 0xfe2ce6e0u)
    LC_MD5_STEP(LC_MD5_I, c, d, a, b, 6, 15, 0xa3014314u) LC_MD5_STEP(LC_MD5_I, b, c, d, a, 13, 21, 0x4e0811a1u)
    LC_MD5_STEP(LC_MD5_I, a, b, c, d, 4, 6, 0xf7537e82u) LC_MD5_STEP(LC_MD5_I, d, a, b, c, 11, 10, 0xbd3af235u)
    LC_MD5_STEP(LC_MD5_I, c, d, a, b, 2, 15, 0x2ad7d2bbu) LC_MD5_STEP(LC_MD5_I, b, c, d, a, 9, 21, 0xeb86d391u)
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
}
#undef LC_MD5_STEP
#undef LC_MD5_F
#undef LC_MD5_G
#undef LC_MD5_H
#undef LC_MD5_I

LC_DESENS_HD uint8_t hexUpper(uint32_t d) { return uint8_t(d < 10 ? '0' + d : 'A' + (d - 10)); }

// MD5(p[0..len)) as 32 UPPER-case hex digits (CalcMD5, core/common/HashUtil.cpp:319-333) at out.  Reads exactly p[0..len).
LC_DESENS_HD void md5Hex(const uint8_t* p, uint32_t len, uint8_t* out) {
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    const uint32_t nBlocks = (len + 8) / 64 + 1;
    for (uint32_t blk = 0; blk < nBlocks; ++blk) {
        uint32_t x[16];
        const uint32_t base = blk * 64;
        if (base + 64 <= len) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 16; ++i) {
                const uint8_t* q = p + base + 4 * i;
                x[i] = uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24;
            }
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 16; ++i) {
                const uint32_t q = base + 4 * uint32_t(i);
                x[i] = md5Byte(p, len, q) | md5Byte(p, len, q + 1) << 8 | md5Byte(p, len, q + 2) << 16 | md5Byte(p, len, q + 3) << 24;
            }
            if (blk == nBlocks - 1) {
                x[14] = len << 3;
                x[15] = len >> 29;
            }
        }
        md5Block(h, x);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < 4; ++w)
        for (int k = 0; k < 4; ++k) {
            const uint32_t byte = (h[w] >> (8 * k)) & 0xFFu;
            out[8 * w + 2 * k] = hexUpper(byte >> 4);
            out[8 * w + 2 * k + 1] = hexUpper(byte & 15u);
        }
}

// ---------------------------------------------------------------------------------------------- one search result -> one cut
// What a value carries between rounds.  from: `const`: where the next search resumes INSIDE the whole value (p); `md5`: where the
// remaining suffix begins (s).  lastEnd: `const` only, the end of the last replaced match (kNone: none yet).  last: the newest record
// of the chain (kNone: no cut, the value is unchanged).
struct ValueState {
    uint32_t from = 0, lastEnd = kNone, last = kNone;
};

// a row no search can have produced is never turned into a write: the value is left alone and reported like one the engine gave up on
LC_DESENS_HD bool refuse(ValueState& S, uint8_t& flags) {
    flags |= kFlagGaveUp;
    S.last = kNone;
    return false;
}

// Applies the method's rule to the result of the search that has just run on a value of n bytes.
//   caps: the engine's row, group g at caps[2 * (g - 1)]: group 1 the whole match, group 2 the `before` group.  `const`: relative to the
//         value (the search was resumed inside it); `md5`: relative to S.from (a fresh search of the suffix).
//   rec:  the record slot recIdx this round holds for the value; written only when a cut is made.
//   refGroup: the engine groups whose spans a record carries (P.nRef of them).
// true: the value takes part in the next round.
LC_DESENS_HD bool collectStep(const Program& P, const uint32_t* refGroup, bool replacingAll, uint32_t n, uint8_t status, const int32_t* caps,
                              ValueState& S, uint32_t recIdx, uint32_t* rec, uint8_t& flags) {
    if (status != kStatusMatch) {
        if (status != 0) return refuse(S, flags);  // LC_GAVE_UP (or a line the engine left undecided): never half-masked, never silent
        return false;
    }
    if (P.method == kMethodConst) {
        // RE2::Replace / GlobalReplace: searches resumed inside the whole value
        const uint32_t mb = uint32_t(caps[0]), me = uint32_t(caps[1]);
        if (caps[0] < 0 || mb < S.from || mb > me || me > n) return refuse(S, flags);
        if (mb == me && mb == S.lastEnd) {  // an empty match right behind the last one: step ONE byte (2018-09-01)
            S.from += 1;
            return S.from <= n;
        }
        rec[0] = S.last;
        rec[1] = mb;
        rec[2] = me;
        for (uint32_t r = 0; r < P.nRef; ++r) {
            const int32_t b = caps[2 * (refGroup[r] - 1)], e = caps[2 * (refGroup[r] - 1) + 1];
            const bool took = b >= 0 && b <= e && uint32_t(e) <= n;  // a group that did not take part gives ""
            rec[kRecHead + 2 * r] = took ? uint32_t(b) : 0u;
            rec[kRecHead + 2 * r + 1] = took ? uint32_t(e) : 0u;
        }
        S.last = recIdx;
        S.from = me;
        S.lastEnd = me;
        return replacingAll;  // (me <= n always holds)
    }
    // FindAndConsume: every search is a fresh search of the remaining suffix
    const uint32_t s = S.from;
    const uint32_t g = s + uint32_t(caps[3]), me = s + uint32_t(caps[1]);
    if (caps[1] < 0 || caps[3] < 0 || g > me || me > n) return refuse(S, flags);
    if (me == s) {  // an empty match at the point of consumption: the WHOLE value stays unchanged, earlier replacements included
        S.last = kNone;
        return false;
    }
    rec[0] = S.last;
    rec[1] = g;
    rec[2] = me;
    S.last = recIdx;
    S.from = me;
    return replacingAll && me < n;
}

// ---------------------------------------------------------------------------------------------- sizes and the writer
LC_DESENS_HD uint32_t replacementLen(const Program& P, const uint32_t* rec) {
    if (P.method == kMethodMd5) return 32;
    uint32_t total = 0;
    for (uint32_t k = 0; k < P.nPieces; ++k) {
        const uint32_t* piece = P.pieces + 3 * k;
        total += piece[0] == kPieceLiteral ? piece[2] : rec[kRecHead + 2 * piece[1] + 1] - rec[kRecHead + 2 * piece[1]];
    }
    return total;
}

// the output length of a value of n bytes from its cut list (64-bit: n replacements of a long rewrite can pass 4 GiB)
LC_DESENS_HD uint64_t outLen(const Program& P, uint32_t n, uint32_t last, const uint32_t* recs) {
    uint64_t total = n;
    const uint32_t W = recWords(P);
    for (uint32_t r = last; r != kNone;) {
        const uint32_t* rec = recs + size_t(r) * W;
        total += replacementLen(P, rec);
        total -= rec[2] - rec[1];
        r = rec[0];
    }
    return total;
}

LC_DESENS_HD void copyBytes(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane, uint32_t stride) {
    for (uint32_t i = lane; i < len; i += stride) dst[i] = src[i];
}

// Lays the value's output (total bytes, outLen() of the same chain) at dst, walking the chain from the newest cut: the tail first, the
// first prefix last.  `stride` callers with lane = 0..stride-1 share the work: every copy is strided over them (neighbouring lanes,
// neighbouring bytes), and the digest of the chain's k-th cut is computed by lane k % stride, `stride` digests at a time.
LC_DESENS_HD void writeValue(const Program& P, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t total, uint32_t last, const uint32_t* recs,
                             uint32_t lane, uint32_t stride) {
    const uint32_t W = recWords(P);
    uint32_t srcEnd = n, outEnd = total, k = 0;
    uint32_t myB = 0, myE = 0, myAt = 0;
    bool mine = false;
    for (uint32_t r = last; r != kNone;) {
        const uint32_t* rec = recs + size_t(r) * W;
        const uint32_t cutB = rec[1], me = rec[2];
        outEnd -= srcEnd - me;
        copyBytes(dst + outEnd, src + me, srcEnd - me, lane, stride);
        if (P.method == kMethodMd5) {
            outEnd -= 32;
            if (k % stride == lane) {
                myB = cutB;
                myE = me;
                myAt = outEnd;
                mine = true;
            }
            if (++k % stride == 0) {
                if (mine) md5Hex(src + myB, myE - myB, dst + myAt);
                mine = false;
            }
        } else {
            for (uint32_t q = P.nPieces; q-- > 0;) {
                const uint32_t* piece = P.pieces + 3 * q;
                if (piece[0] == kPieceLiteral) {
                    outEnd -= piece[2];
                    copyBytes(dst + outEnd, P.lit + piece[1], piece[2], lane, stride);
                } else {
                    const uint32_t b = rec[kRecHead + 2 * piece[1]], e = rec[kRecHead + 2 * piece[1] + 1];
                    outEnd -= e - b;
                    copyBytes(dst + outEnd, src + b, e - b, lane, stride);
                }
            }
        }
        srcEnd = cutB;
        r = rec[0];
    }
    if (mine) md5Hex(src + myB, myE - myB, dst + myAt);
    copyBytes(dst, src, srcEnd, lane, stride);  // (outEnd == srcEnd here)
}

}  // namespace lcdesens

// ---------------------------------------------------------------------------------------------- host only: the rewrite parser, the walk
#include <string>
#include <vector>

namespace lcdesens {

struct ParsedRewrite {
    std::vector<uint32_t> pieces;    // three words each
    std::vector<uint8_t> lit;        // the literal pieces' bytes
    std::vector<uint32_t> refGroup;  // ENGINE groups whose spans a record carries, by slot
    bool passThrough = false;        // RE2's error path: a backslash in front of anything but 0-9 and '\' (or at the end)
    uint32_t maxEngineGroup = 2;     // what the match calls must report (the whole match and the `before` group at least)
};

// RE2::Rewrite's reading of a rewrite string (re2.cc, 2018-09-01): \0..\9 name RE2's groups (RE2 group k = engine group k + 1, the
// engine's group 1 being the whole match), "\\" is a backslash, every other byte is itself.  A number above the pattern's group count
// gives "" (that release's rule), so such a piece is dropped here.  re2Groups: the capturing groups of "(before)content".
inline ParsedRewrite parseRewrite(const std::string& rewrite, int re2Groups) {
    ParsedRewrite out;
    const auto literal = [&](uint8_t c) {
        const size_t np = out.pieces.size();
        if (np && out.pieces[np - 3] == kPieceLiteral && out.pieces[np - 2] + out.pieces[np - 1] == out.lit.size()) {
            ++out.pieces[np - 1];
        } else {
            out.pieces.push_back(kPieceLiteral);
            out.pieces.push_back(uint32_t(out.lit.size()));
            out.pieces.push_back(1);
        }
        out.lit.push_back(c);
    };
    for (size_t i = 0; i < rewrite.size(); ++i) {
        const uint8_t c = uint8_t(rewrite[i]);
        if (c != '\\') {
            literal(c);
            continue;
        }
        if (i + 1 >= rewrite.size()) {
            out.passThrough = true;
            return out;
        }
        const uint8_t d = uint8_t(rewrite[++i]);
        if (d == '\\') {
            literal('\\');
        } else if (d >= '0' && d <= '9') {
            const int k = d - '0';
            if (k > re2Groups) continue;
            const uint32_t g = uint32_t(k) + 1;
            uint32_t slot = 0;
            while (slot < out.refGroup.size() && out.refGroup[slot] != g) ++slot;
            if (slot == out.refGroup.size()) out.refGroup.push_back(g);
            if (g > out.maxEngineGroup) out.maxEngineGroup = g;
            out.pieces.push_back(kPieceGroup);
            out.pieces.push_back(slot);
            out.pieces.push_back(g);
        } else {
            out.passThrough = true;
            return out;
        }
    }
    return out;
}

inline Program programOf(uint32_t method, const ParsedRewrite& R) {
    Program P;
    P.method = method;
    if (method == kMethodConst) {
        P.nPieces = uint32_t(R.pieces.size() / 3);
        P.nRef = uint32_t(R.refGroup.size());
        P.pieces = R.pieces.data();
        P.lit = R.lit.data();
    }
    return P;
}

// One value on the host, the way the device does it in rounds: search(from, fresh, caps) answers one search -- `const`: of the whole
// value resumed at `from`; `md5` (fresh): of value[from:] on its own -- with the engine's status and row.  -> changed; out = the new value.
template <class Search>
bool walkValue(const Program& P, const ParsedRewrite& R, bool replacingAll, const uint8_t* value, uint32_t n, uint32_t nGroups, Search search,
               std::vector<uint8_t>& out, uint8_t* flagsOut = nullptr, uint32_t* roundsOut = nullptr) {
    ValueState S;
    std::vector<uint32_t> recs;
    std::vector<int32_t> caps(2 * size_t(nGroups));
    const uint32_t W = recWords(P);
    uint8_t flags = 0;
    uint32_t rounds = 0;
    for (bool again = true; again;) {
        caps.assign(caps.size(), -1);
        const uint8_t status = search(S.from, P.method == kMethodMd5, caps.data());
        const uint32_t recIdx = uint32_t(recs.size() / W);
        recs.resize(recs.size() + W);
        again = collectStep(P, R.refGroup.data(), replacingAll, n, status, caps.data(), S, recIdx, recs.data() + size_t(recIdx) * W, flags);
        // every round either cuts behind the last cut or steps a byte, so a value of n bytes is through after 2n + 2 searches; a walk
        // that is not has lost that property (a changed rule) and says so instead of spinning
        if (++rounds > 2 * uint64_t(n) + 4) {
            again = refuse(S, flags);
        }
    }
    if (roundsOut) *roundsOut = rounds;
    if (S.last != kNone) flags |= kFlagChanged;
    if (flagsOut) *flagsOut = flags;
    if (S.last == kNone) return false;
    const uint64_t total = outLen(P, n, S.last, recs.data());
    out.assign(size_t(total), 0);
    writeValue(P, value, n, out.data(), uint32_t(total), S.last, recs.data(), 0, 1);
    return true;
}

}  // namespace lcdesens
