// codec_kernel.hpp -- the gfx950 kernels of the field codecs (include/codec/lc_codec.h; wave64), included by codec_device.hip only.  The
// per-unit rules are codec_vm.hpp's, shared with the host; the scan between a size pass and a write pass is scan64_kernel.hpp's.
//
//   codec_len_kernel         encode and MD5: flags, output lengths and the scan's input (encode) or the offsets themselves (MD5: a
//                            fixed stride of 32 bytes, no scan) from the input lengths alone.
//   b64_encode_kernel        kLanes lanes per value.  A lane takes units of 12 input bytes and gives 16 characters.  The 12 bytes lie
//                            anywhere: the lane loads the (up to four) ALIGNED words that hold them -- only words that hold a byte of
//                            the value, so every load stays inside the 16-byte units the value touches, the read contract of d_data --
//                            and funnel-shifts them into place.  A value's output begins 16-byte aligned, so a full unit is ONE 16-byte
//                            store and the last unit is one to four word stores.  No byte stores.
//   b64_decode_size_kernel   one value per lane through the SOURCE of wave_tile_source.hpp, unchanged (a wavefront owns 64 rows x 64
//                            bytes of LDS, stage s + 1 in flight while the lanes walk stage s).  Per 16-byte unit of its row a lane runs
//                            b64DecodeUnit; the state that crosses units is five registers.  It writes the flags, the error offset, the
//                            output length, the scan's input and the CLEAN byte (no CR/LF in the value).  Nothing else: the write pass
//                            ranks the significant characters of a value with CR/LF itself, walking the value in order.
//   b64_decode_write_kernel  kLanes lanes per value; a value without output ends at once.
//                            CLEAN: a lane takes 16 characters (aligned words + funnel shift, as above) and gives 12 bytes: three
//                            aligned word stores.  Only the last unit's tail of 1 to 3 bytes uses byte stores.
//                            With CR/LF: the sub-group walks the value 64 bytes a round, one byte per lane and step; a ballot of "is an
//                            alphabet byte" and a popcount of the lower lanes' bits rank the byte, its sextet is staged at its rank in
//                            LDS (96 bytes per sub-group), and whole staged units are converted as above.
//   md5_field_kernel         one value per lane through the same SOURCE, one 64-byte block per step.  A value's bytes begin `head`
//                            bytes into its first stage, so block j is the last 64 - head bytes of stage j and the first head bytes
//                            of stage j + 1: the lane keeps stage j's sixteen words in registers, selects by head / 4 (two rounds of
//                            conditional moves, static indices) and funnel-shifts by head % 4.  Padding is applied per word
//                            (md5PaddedWord), so whatever stands behind the value is never hashed.  32 hex digits = two 16-byte stores.
// Nothing is stored outside [out_off[i], out_off[i] + out_len[i]), nothing at all when out_off[n] exceeds out_cap.
// Plain C++ loads and stores only.  DESIGN.md section 5.22 has the resource report.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "codec_vm.hpp"
#include "wave_tile_source.hpp"

namespace lccodec {

constexpr int kBlock = 256;
constexpr uint32_t kTileBytes = lcwave::kWaveTileBytes;  // per wavefront
constexpr uint32_t kStagedWords = 24;                     // per sub-group of the decode write pass: 15 sextets left over + 64 new ones

typedef uint8_t __attribute__((address_space(3))) * LdsBytePtr;

// lo | hi << 32, shifted right by sh bytes (0..3)
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh) { return uint32_t(((uint64_t(hi) << 32) | lo) >> (8 * sh)); }

// the kWords + 1 aligned words that hold the `need` bytes (>= 1) at addr, shifted into place: w[0 .. kWords).  Only words that hold one
// of the bytes are loaded.
template <uint32_t kWords>
__device__ __forceinline__ void loadShifted(uintptr_t addr, uint32_t need, uint32_t w[kWords]) {
    const uint32_t sh = uint32_t(addr & 3u);
    const uint32_t* base = reinterpret_cast<const uint32_t*>(addr - sh);
    uint32_t d[kWords + 1];
#pragma unroll
    for (uint32_t j = 0; j <= kWords; ++j) d[j] = 4 * j < sh + need ? base[j] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kWords; ++j) w[j] = funnel(d[j], d[j + 1], sh);
}

__global__ __launch_bounds__(kBlock) void codec_len_kernel(uint32_t op, const uint32_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ flags,
                                                          uint64_t* __restrict__ outOff, uint32_t* __restrict__ outLen) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i == n) outOff[n] = op == kCodecMd5 ? 32ull * n : 0ull;
    if (i >= n) return;
    const uint32_t len = off[i + 1] - off[i];
    flags[i] = kCodecFlagOut;
    if (op == kCodecMd5) {
        outLen[i] = 32;
        outOff[i] = 32ull * i;
    } else {
        const uint32_t chars = codecEncodedLen(len);
        outLen[i] = chars;
        outOff[i] = (uint64_t(chars) + 15u) & ~15ull;  // (the scan's input)
    }
}

template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void b64_encode_kernel(const uint8_t* __restrict__ data, const uint32_t* __restrict__ off, uint32_t n,
                                                           const uint64_t* __restrict__ outOff, uint8_t* __restrict__ out, uint64_t outCap) {
    static_assert(kLanes >= 1 && kLanes <= 64 && (kLanes & (kLanes - 1)) == 0, "lanes per value: a divisor of 64");
    if (outOff[n] > outCap) return;  // too small: not one byte is stored
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    const uint32_t lane = threadIdx.x % kLanes;
    if (i64 >= n) return;
    const uint32_t i = uint32_t(i64);
    const uint32_t at = off[i], len = off[i + 1] - at;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(data) + at;
    const uint32_t units = (len + 11) / 12;
    uint8_t* dst = out + outOff[i];  // 16-byte aligned
    for (uint32_t u = lane; u < units; u += kLanes) {
        const uint32_t r = len - 12 * u;
        uint32_t w[3], o[4];
        loadShifted<3>(addr + 12 * u, r < 12u ? r : 12u, w);
        if (r >= 12) {
            b64Encode12(w, o);
            *reinterpret_cast<lcwave::u32x4*>(dst + 16 * u) = lcwave::u32x4{o[0], o[1], o[2], o[3]};
        } else {
            const uint32_t words = b64EncodeTail(w, r, o);
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + 16 * u);
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g)
                if (g < words) d[g] = o[g];
        }
    }
}

// sizes: uint64[n + 1] (the scan's input: sizes[n] = 0); errOff may be null
__global__ __launch_bounds__(kBlock) void b64_decode_size_kernel(const uint8_t* __restrict__ data, const uint32_t* __restrict__ off, uint32_t n,
                                                                uint8_t* __restrict__ flags, uint32_t* __restrict__ errOff, uint64_t* __restrict__ sizes,
                                                                uint32_t* __restrict__ outLen, uint8_t* __restrict__ clean) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t line64 = uint64_t(blockIdx.x) * kBlock + tid;
    const bool live = line64 < n;
    const uint32_t line = live ? uint32_t(line64) : 0u;
    if (line64 == n) sizes[n] = 0;
    uint32_t at = 0, len = 0;
    if (live) {
        at = off[line];
        len = off[line + 1] - at;
    }
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsBytePtr)tiles)) + wave * kTileBytes;  // LDS byte address
    lcwave::WaveTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    const uint32_t head = src.head(), end = head + len;
    B64DecodeState state;
    const uint32_t stages = src.stageCount(len ? end : 0u);
    for (uint32_t s = 0; s < stages; ++s) {
        src.stage(s);
        const uint32_t base = s * lcwave::kWaveStageBytes;
        if (base >= end || !len) continue;  // this lane's value has ended: it only takes part in the cooperative stages
#pragma unroll 1
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ub = base + k * 16;
            if (ub >= end) break;
            uint32_t q[4];
            src.rowQuad(k, q);
            b64DecodeUnit(state, q, ub < head ? head - ub : 0u, end - ub < 16u ? end - ub : 16u, ub - head);
        }
    }
    if (!live) return;
    uint32_t bytes, where;
    const uint32_t f = b64DecodeFinish(state, len, &bytes, &where);
    flags[line] = uint8_t(f);
    outLen[line] = bytes;
    sizes[line] = codecRound16(bytes);
    clean[line] = state.sawSkip ? 0 : 1;
    if ((f & kCodecFlagError) && errOff) errOff[line] = where;
}

// one unit's bytes: words where a whole word is the value's, bytes for the value's last 1 to 3
__device__ __forceinline__ void storeDecoded(uint8_t* dst, const uint32_t o[3], uint32_t bytes) {
#pragma unroll
    for (uint32_t g = 0; g < 3; ++g) {
        if (4 * g + 4 <= bytes) {
            *reinterpret_cast<uint32_t*>(dst + 4 * g) = o[g];
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 3; ++b)
                if (4 * g + b < bytes) dst[4 * g + b] = uint8_t(o[g] >> (8 * b));
        }
    }
}

template <uint32_t kLanes>
__global__ __launch_bounds__(kBlock) void b64_decode_write_kernel(const uint8_t* __restrict__ data, const uint32_t* __restrict__ off, uint32_t n,
                                                                 const uint8_t* __restrict__ flags, const uint8_t* __restrict__ clean,
                                                                 const uint64_t* __restrict__ outOff, const uint32_t* __restrict__ outLen,
                                                                 uint8_t* __restrict__ out, uint64_t outCap) {
    static_assert(kLanes >= 4 && kLanes <= 64 && (kLanes & (kLanes - 1)) == 0, "lanes per value: a divisor of 64");
    __shared__ __attribute__((aligned(16))) uint32_t staged[(kBlock / kLanes) * kStagedWords];
    if (outOff[n] > outCap) return;  // too small: not one byte is stored
    const uint64_t i64 = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kLanes;
    const uint32_t lane = threadIdx.x % kLanes;
    if (i64 >= n) return;
    const uint32_t i = uint32_t(i64);
    if (!(flags[i] & kCodecFlagOut)) return;  // (the same in every lane of the sub-group)
    const uint32_t bytes = outLen[i];
    if (!bytes) return;
    const uint32_t at = off[i], len = off[i + 1] - at;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(data) + at;
    const uint32_t sextets = b64SextetsOf(bytes), units = (sextets + 15) / 16;
    uint8_t* dst = out + outOff[i];  // 16-byte aligned; a unit's 12 bytes keep word alignment
    if (clean[i]) {
        // the value's first `sextets` bytes ARE its significant characters
        for (uint32_t u = lane; u < units; u += kLanes) {
            const uint32_t m = sextets - 16 * u < 16u ? sextets - 16 * u : 16u;
            uint32_t c[4], s[4], o[3];
            loadShifted<4>(addr + 16 * u, m, c);
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) s[g] = b64Sextets4(c[g]);
            b64Decode16(s, o);
            storeDecoded(dst + 12 * u, o, b64UnitBytes(m));
        }
        return;
    }
    // with CR/LF: rank, stage, convert
    uint32_t* mine = staged + (threadIdx.x / kLanes) * kStagedWords;
    uint8_t* mineBytes = reinterpret_cast<uint8_t*>(mine);
    const uint32_t shift = (threadIdx.x & 63u) / kLanes * kLanes;  // where the sub-group's bits begin in a ballot
    const uint64_t groupMask = kLanes == 64 ? ~0ull : (1ull << kLanes) - 1ull;
    const uint8_t* value = reinterpret_cast<const uint8_t*>(addr);
    uint32_t carry = 0, doneUnits = 0;
    for (uint32_t base = 0; base < len; base += 64) {  // a round of the sub-group (the same trip count in all of its lanes)
#pragma unroll
        for (uint32_t step = 0; step < 64 / kLanes; ++step) {
            const uint32_t p = base + step * kLanes + lane;
            const uint32_t cls = p < len ? b64Class(value[p]) : kB64Other;
            const bool significant = cls < 64u;
            const uint64_t bits = (__ballot(significant) >> shift) & groupMask;
            const uint32_t rank = carry + uint32_t(__popcll(bits & ((1ull << lane) - 1ull)));
            if (significant) mineBytes[rank] = uint8_t(cls);
            carry += uint32_t(__popcll(bits));
        }
        lcwave::waveLdsSync();
        const uint32_t full = carry >> 4, left = carry & 15u;
        if (lane < full && doneUnits + lane < units) {  // (the bound: what the size pass counted)
            const uint32_t s[4] = {mine[4 * lane], mine[4 * lane + 1], mine[4 * lane + 2], mine[4 * lane + 3]};
            uint32_t o[3];
            b64Decode16(s, o);
            storeDecoded(dst + 12 * (doneUnits + lane), o, 12);
        }
        // the sextets left over go to the front
        uint32_t moved = 0;
        if (full && lane < left) moved = mineBytes[16 * full + lane];
        lcwave::waveLdsSync();
        if (full && lane < left) mineBytes[lane] = uint8_t(moved);
        lcwave::waveLdsSync();
        doneUnits += full;
        carry = left;
    }
    if (carry && lane == 0 && doneUnits == units - 1) {  // the value's last unit: 2 to 15 sextets
        const uint32_t s[4] = {mine[0], mine[1], mine[2], mine[3]};
        uint32_t o[3];
        b64Decode16(s, o);
        storeDecoded(dst + 12 * doneUnits, o, b64UnitBytes(sextets - 16 * doneUnits < carry ? sextets - 16 * doneUnits : carry));
    }
}

// out: 32 bytes per value at 32 * i
__global__ __launch_bounds__(kBlock) void md5_field_kernel(const uint8_t* __restrict__ data, const uint32_t* __restrict__ off, uint32_t n,
                                                          uint8_t* __restrict__ out, uint64_t outCap) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[(kBlock / 64) * kTileBytes];
    if (32ull * n > outCap) return;  // too small: not one byte is stored
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t line64 = uint64_t(blockIdx.x) * kBlock + tid;
    const bool live = line64 < n;
    const uint32_t line = live ? uint32_t(line64) : 0u;
    uint32_t at = 0, len = 0;
    if (live) {
        at = off[line];
        len = off[line + 1] - at;
    }
    const uint32_t tile = uint32_t(reinterpret_cast<uintptr_t>((LdsBytePtr)tiles)) + wave * kTileBytes;  // LDS byte address
    lcwave::WaveTileSource src(lane, tile, reinterpret_cast<uintptr_t>(data) + at);
    const uint32_t head = src.head(), end = head + len;
    const uint32_t blocks = live ? md5Blocks(len) : 0u;
    const uint32_t stages = src.stageCount(len ? end : 0u);  // (at most the longest value's blocks + 1)
    uint32_t longest = blocks;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t other = __shfl_xor(longest, d, 64);
        longest = other > longest ? other : longest;
    }
    longest = __builtin_amdgcn_readfirstlane(longest);
    const uint32_t skipWords = head >> 2, skipBytes = head & 3u;
    uint32_t h[4];
    md5Init(h);
    // (every index below is a constant in the source, not a loop variable: the arrays must be registers before any pass can turn a
    // select between two of their elements into one load at a computed address, which would put them into scratch)
#define LC_CODEC_REP16(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
    uint32_t cat[20];  // the stage before (16 words) and the first four of the current one
    uint32_t cur[16];
#define LC_CODEC_ZERO(d) cur[d] = 0;
    LC_CODEC_REP16(LC_CODEC_ZERO)
    const bool skipTwo = (skipWords & 2u) != 0, skipOne = (skipWords & 1u) != 0;
    for (uint32_t it = 0; it <= longest; ++it) {
#define LC_CODEC_KEEP(d) cat[d] = cur[d];
        LC_CODEC_REP16(LC_CODEC_KEEP)
        if (it < stages) {
            src.stage(it);
            const lcwave::u32x4 q0 = *reinterpret_cast<lcwave::LdsQuadPtr>(src.myRow + (0u ^ src.mySwizzle));
            const lcwave::u32x4 q1 = *reinterpret_cast<lcwave::LdsQuadPtr>(src.myRow + (16u ^ src.mySwizzle));
            const lcwave::u32x4 q2 = *reinterpret_cast<lcwave::LdsQuadPtr>(src.myRow + (32u ^ src.mySwizzle));
            const lcwave::u32x4 q3 = *reinterpret_cast<lcwave::LdsQuadPtr>(src.myRow + (48u ^ src.mySwizzle));
            cur[0] = q0.x, cur[1] = q0.y, cur[2] = q0.z, cur[3] = q0.w;
            cur[4] = q1.x, cur[5] = q1.y, cur[6] = q1.z, cur[7] = q1.w;
            cur[8] = q2.x, cur[9] = q2.y, cur[10] = q2.z, cur[11] = q2.w;
            cur[12] = q3.x, cur[13] = q3.y, cur[14] = q3.z, cur[15] = q3.w;
        }
        cat[16] = cur[0], cat[17] = cur[1], cat[18] = cur[2], cat[19] = cur[3];
        if (it >= 1 && it - 1 < blocks) {
            uint32_t two[18], one[17], x[16];
#define LC_CODEC_TWO(d) two[d] = skipTwo ? cat[d + 2] : cat[d];
            LC_CODEC_REP16(LC_CODEC_TWO) LC_CODEC_TWO(16) LC_CODEC_TWO(17)
#define LC_CODEC_ONE(d) one[d] = skipOne ? two[d + 1] : two[d];
            LC_CODEC_REP16(LC_CODEC_ONE) LC_CODEC_ONE(16)
#define LC_CODEC_FUNNEL(d) x[d] = funnel(one[d], one[d + 1], skipBytes);
            LC_CODEC_REP16(LC_CODEC_FUNNEL)
#define LC_CODEC_PAD(d) x[d] = md5PaddedWord(x[d], 64u * (it - 1) + 4u * d, len);
            LC_CODEC_REP16(LC_CODEC_PAD)
            if (it == blocks) {  // the last block carries the length
                x[14] = len << 3;
                x[15] = len >> 29;
            }
            lcdesens::md5Block(h, x);
        }
    }
#undef LC_CODEC_REP16
#undef LC_CODEC_ZERO
#undef LC_CODEC_KEEP
#undef LC_CODEC_TWO
#undef LC_CODEC_ONE
#undef LC_CODEC_FUNNEL
#undef LC_CODEC_PAD
    if (!live) return;
    uint32_t o[8];
    md5HexLower(h, o);
    lcwave::u32x4* dst = reinterpret_cast<lcwave::u32x4*>(out + 32ull * line);
    dst[0] = lcwave::u32x4{o[0], o[1], o[2], o[3]};
    dst[1] = lcwave::u32x4{o[4], o[5], o[6], o[7]};
}

}  // namespace lccodec
