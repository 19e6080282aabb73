// tdfa_kernel.hpp -- device pieces of the tagged-DFA engine's LDS kernels (tdfa_stream_kernel.hpp): layout constants, the
// general-program replay, the result epilogue, the completion signal.
//
// One log line per lane, 64 lines per wavefront, tables in LDS.
//
// HBM side.  A lane walking its own line with its own loads touches a different cache line per lane per load, and
// with enough wavefronts in flight the lines are evicted from L2 between two visits (measured: 2.6-3.4x the
// algorithmic bytes fetched, the kernel then sits on the HBM ceiling doing wasted traffic).  So the wavefront
// loads COOPERATIVELY: per stage, four lanes fetch 64 contiguous bytes of one line (16 lines per
// global_load_dwordx4, 4 loads per stage), the 64x64-byte tile goes to a per-wave LDS staging buffer, and each lane
// then reads its own row back with ds_read_b128.  Every byte is fetched from HBM once, in 64-byte runs.  The next
// stage's loads are in flight (in VGPRs) while the current stage is stepped.  Only the wavefront itself touches
// its staging rows, so no workgroup barrier is involved.
//
// LDS side.  A stage is stepped in aligned 16-byte chunks; every chunk in three phases so that the only serial
// dependency is the DFA state itself:
//   phase 0  class lookups   col[j] = cmap8[byte j]                       16 x (v_add_sdwa + ds_read_u8), independent
//   phase 1  state chain     t = lds32[(t & 0xFFFF) + col[j]]             16 x (v_add_sdwa + ds_read_b32), dependent;
//                            the low half of a transition entry IS the LDS address of the next state's row
//   phase 2  capture writes  regs[(t_j >> 16)][lane] = pos_j              16 x (v_add_sdwa + v_add + ds_write_b32), independent;
//                            the high half of an entry IS the LDS offset of the offset register the transition
//                            stamps; transitions that stamp nothing point at a dummy register, so phase 2 has no
//                            branches and no divergence (lines hit group boundaries at different bytes: a
//                            branch per byte would be taken by some lane almost every byte)
// Transitions whose register program is more than "one register = pos" (rare for log regexes) carry a list id
// and a flag instead; a wave that saw such a flag anywhere in the chunk replays the chunk in order, with branches.
// Capture-offset registers live in LDS as regs[reg][lane]: the register number is data dependent (VGPRs would
// need scratch indexing) and [reg][lane] is bank-conflict free.
//
// Bytes outside the lane's line (head of the first aligned chunk, tail of the last, stages past the end of a
// short line) take the row's identity column.  When every lane of the wavefront is in the middle of its line a
// wave-uniform branch skips the validity selects.  Loads are aligned 16-byte segments that contain at least one
// byte of the line, so none can leave the line's pages.
//
// COMPACT variants (regex_handle.cpp packTdfaWideBlob: 256 lanes by default for large batches): 16-bit offset registers (lines of 64 KiB and more are left to a second launch
// of the 32-bit kernel) and an unpadded, XOR-swizzled staging tile -- 106 instead of 164 bytes of LDS per line, i.e. more
// lines in flight per CU.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/lc_regex_gpu.h"
#include "device_tables.h"

#ifndef LC_TDFA_MIN_WAVES
#define LC_TDFA_MIN_WAVES 1  // waves per SIMD the register allocator must leave room for
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t __attribute__((address_space(3))) * LdsWordPtr;
typedef u32x4 __attribute__((address_space(3))) * LdsQuadPtr;
typedef const uint8_t __attribute__((address_space(3))) * LdsBytePtr;
typedef const u32x4 __attribute__((address_space(1))) * GlobalQuadPtr;

// capture offsets are 32-bit (a line may be as long as a 512 KiB read buffer); the COMPACT variants keep 16-bit ones
template <typename RegT>
using LdsRegPtrT = RegT __attribute__((address_space(3))) *;
constexpr uint32_t kTdfaWideMaxLine = 0xFFFFu;  // longest line the COMPACT variants take

#ifndef LC_TDFA_STAGE_BYTES
#define LC_TDFA_STAGE_BYTES 64
#endif
constexpr uint32_t kTdfaStageBytes = LC_TDFA_STAGE_BYTES;  // bytes of each line staged per round (32 or 64)
constexpr int kTdfaLoads = int(kTdfaStageBytes / 16);       // loads per stage == lanes that share one line
constexpr uint32_t kTdfaRowStride = kTdfaStageBytes + 16;  // +16: rows 20 dwords apart -> conflict-free b128 reads
constexpr uint32_t kTdfaStagePerWave = 64 * kTdfaRowStride;

__device__ __forceinline__ void tdfaWaveLdsSync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Measurement variants (tools/tdfa_lab.hip instantiates them; the product instantiates LAB = 0 and, for tables that carry no
// general register program at all -- device_tables.h TD_NREGS_NO_GENERAL --, kTdfaNoGeneralPrograms).  They answer "what
// does each of the three LDS instructions per byte cost" on the real kernel instead of a model of it:
//   kLabNoStamp    phase 2 is skipped (capture offsets come out wrong: timing only); with kLabPairOne: no stamp and no settled doubles
//   kLabPreClass   the input bytes ARE column offsets already (host pre-classified copy of the corpus): no class lookup
//   kLabGlobalClass the class lookup goes to the 256-byte map in global memory (vector L1) instead of LDS
//   kLabReplicated the transition table is stored 16 times, entry e of replica r at ((e * 16) + r) * 4: lane l reads replica
//                  l & 15, so the 32 lanes of an LDS lane group touch 16 banks at most twice -- no chain bank conflicts
//   kLabNoOutput / kLabNoLoop (tdfa_stream_kernel only): skip the capture-table write / the stage loop -- what a workgroup's
//                  fixed costs are (line table reads, first loads, table staging, result write)
//   kLabNoGeneral  (tdfa_stream_kernel only): no check for general register programs (wrong for tables that have one on the
//                  walked path): what the check costs -- and what tables without such programs need not pay
enum { kLabNoStamp = 1, kLabPreClass = 2, kLabGlobalClass = 4, kLabReplicated = 8, kLabNoOutput = 16, kLabNoLoop = 32, kLabNoGeneral = 64,
       kLabOneStamp = 128 /* byte-pair chunks only: one stamp per pair (timing only) */,
       kLabDmaStage = 256 /* tdfa_stream_kernel, COMPACT: the staging tile is filled by global_load_lds_dwordx4 (no staging VGPRs) */,
       kLabWaves5 = 512 /* tdfa_stream_kernel: register budget of 5 waves per SIMD (96 VGPRs) */,
       kLabNoDmaWait = 1024 /* DMA staging without the wait for the stage (wrong bytes: timing only -- what the wave loses there) */,
       kLabPairOne = 4096 /* byte-pair chunks on a ONE-STAMP pair table (device_tables.h TP1_*, LC_TDFA_PAIR=2): exact */,
       kLabMopUp = 8192 /* tdfa_stream_kernel: the launch behind a COMPACT one -- a small grid whose workgroups take the line blocks in turn */,
       kLabDeferStamps = 16384 /* one-stamp pair kernel, COMPACT: stamps wait in two VGPRs per lane until some lane holds two (exact) */ };
constexpr int kTdfaNoGeneralPrograms = kLabNoGeneral;  // the product's second instantiation (gpu_runtime.hip launchTdfaBlock)

// general register program (a list of moves); rare for log regexes
// Column of a lane in the register file.  32-bit registers: the lane itself (a wavefront's lanes hit 32 banks twice over, one
// half-wave after the other).  16-bit registers: lanes l and l+32 share a dword -- two NEIGHBOURING lanes in one dword stamp
// different registers most of the time, i.e. different dwords of one bank in the same LDS pass: a conflict on nearly every
// stamp (measured: stamps + class lookups add 1.3 conflict cycles per byte-step).
template <typename TdfaReg>
__device__ __forceinline__ uint32_t tdfaRegLane(uint32_t tid) {
    if constexpr (sizeof(TdfaReg) == 2) return (tid & ~63u) | ((tid & 31u) << 1) | ((tid >> 5) & 1u);
    else return tid;
}

template <int BLOCK, typename TdfaReg>
__device__ __forceinline__ void tdfaRunMoveList(uint8_t* smem, uint32_t regsBase, uint32_t list, uint32_t pos,
                                                uint32_t tid) {
    TdfaReg* regs = reinterpret_cast<TdfaReg*>(smem + regsBase);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(smem);
    const uint32_t* opsStart = reinterpret_cast<const uint32_t*>(smem + hdr[TD_OFF_OPSSTART]);
    const uint16_t* ops = reinterpret_cast<const uint16_t*>(smem + hdr[TD_OFF_OPS]);
    const uint32_t at = opsStart[list];
    const uint32_t cnt = ops[at];
#pragma unroll 1
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t w = ops[at + 1 + i];
        const uint32_t dst = w & 0xFF, src = w >> 8;
        const TdfaReg val = (src == TD_REG_POS) ? TdfaReg(pos) : regs[src * BLOCK + tdfaRegLane<TdfaReg>(tid)];
        regs[dst * BLOCK + tdfaRegLane<TdfaReg>(tid)] = val;
    }
}

// a + (t & 0xFFFF)   -- one VALU: SDWA selects the low word of t
__device__ __forceinline__ uint32_t addLowHalf(uint32_t a, uint32_t t) {
    uint32_t r;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
        : "=v"(r)
        : "v"(a), "v"(t));
    return r;
}
// a + (t >> 16)
__device__ __forceinline__ uint32_t addHighHalf(uint32_t a, uint32_t t) {
    uint32_t r;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
        : "=v"(r)
        : "v"(a), "v"(t));
    return r;
}

// In-order replay of one chunk for wavefronts that met a general register program in it: re-walks the 16 bytes
// from the chunk's entry state and applies every register program at its own byte.  Rolled up: it is rare.
template <int BLOCK, typename TdfaReg, int LAB = 0>
__device__ __forceinline__ void tdfaReplayChunk(uint8_t* smem, u32x4 q, uint32_t t, uint32_t base, uint32_t L,
                                                uint32_t idCol, uint32_t regsBase, uint32_t tid, uint32_t nBytes) {
    typedef LdsRegPtrT<TdfaReg> LdsRegPtr;
    const LdsBytePtr cmap = reinterpret_cast<LdsBytePtr>(TD_CMAP_OFFSET);
    const uint32_t regAddr0 = regsBase + tdfaRegLane<TdfaReg>(tid) * sizeof(TdfaReg);
#pragma unroll 1
    for (uint32_t j = 0; j < nBytes; ++j) {
        const uint32_t word = (j < 8) ? ((j < 4) ? q.x : q.y) : ((j < 12) ? q.z : q.w);
        const uint32_t b = (word >> ((j & 3) * 8)) & 0xFFu;
        uint32_t col = (base + j < L) ? ((LAB & kLabPreClass) ? b : uint32_t(cmap[b])) : idCol;
        if constexpr ((LAB & kLabReplicated) != 0) col = (col << 4) + ((tid & 15u) << 2);
        t = *reinterpret_cast<LdsWordPtr>(addLowHalf(col, t));
        if (t & (TD_OP_GENERAL << 16)) tdfaRunMoveList<BLOCK, TdfaReg>(smem, regsBase, t >> 17, base + j, tid);
        else *reinterpret_cast<LdsRegPtr>(addHighHalf(regAddr0, t)) = TdfaReg(base + j);
    }
}

// Tables whose multi-stamp register programs were folded into set registers (regex_handle.cpp, planTdfaFold; the fold words
// of device_tables.h TD_NREGS) read a register as the LARGEST of itself and its sets' registers: every register starts at 0.
template <int BLOCK>
__device__ __forceinline__ void tdfaClearRegisters(uint8_t* smem, const uint32_t* __restrict__ blob, uint32_t blobBytes,
                                                   uint32_t regBytes) {
    if ((blob[TD_NREGS] >> 16) & 0x1FFFu) {  // (wave-uniform: a scalar load of the header word)
        uint32_t* regs = reinterpret_cast<uint32_t*>(smem + blobBytes);
        for (uint32_t i = threadIdx.x; i < regBytes / 4; i += BLOCK) regs[i] = 0;
    }
}

// The result of a wavefront's 64 lines: status byte + 2*nGroupsOut capture offsets per line.  A lane storing its own row
// dword by dword touches 64 different cache lines per store instruction (rows are 8*G bytes apart): measured on the headline
// batch that write alone took a third of the kernel (tools/tdfa_lab.hip, "no output" variant).  When the wave's lines are
// consecutive in the capture table (no schedule permutation, every lane decides its line) the rows form ONE contiguous
// region, so they go through the wave's staging tile (free once the line is walked): lanes write their rows to LDS, then the
// wave copies the region out 256 contiguous bytes per store instruction.  `state` = final DFA state of the lane's line.
template <int BLOCK, typename TdfaReg, int LAB = 0>
__device__ __forceinline__ void tdfaWriteResults(uint8_t* smem, uint32_t tileAddr, uint32_t regsBase, uint32_t state, bool live,
                                                 uint32_t line, uint32_t L, uint32_t from, bool permuted, uint32_t nGroupsOut,
                                                 int32_t* __restrict__ caps, uint8_t* __restrict__ status) {
    // Round 3: this epilogue was a chain of ~100 dependent LDS round trips per wave (a map byte, then a register, per slot and
    // pass; a dword per lane and store in the copy) -- 9 % of the kernel with nothing to overlap it when the workgroups of a CU
    // run in lockstep.  Now: the wave-uniform words (fold words, slot map) are read ONCE, one per lane, and handed round with
    // v_readlane; registers are read eight at a time; the tile leaves in 16-byte pieces.
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(smem);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nSlots = hdr[TD_NSLOTS];
    const uint16_t* finalId = reinterpret_cast<const uint16_t*>(smem + hdr[TD_OFF_FINALID]);
    const uint8_t* finalMap = smem + hdr[TD_OFF_FINALMAP];
    const TdfaReg* regs = reinterpret_cast<const TdfaReg*>(smem + regsBase);
    const uint32_t fid = live ? uint32_t(finalId[state]) : 0xFFFFu;
    const bool matched = live && (state != 0) && (fid != 0xFFFFu);
    const uint32_t nOut = 2 * nGroupsOut;
    const uint32_t rl = tdfaRegLane<TdfaReg>(tid);
    const uint32_t foldOff = ((hdr[TD_NREGS] >> 16) & 0x1FFFu) * 16;
    if (foldOff) {
        // folded multi-stamp programs: a member register reads as the larger of itself and its set's register ("latest stamp"
        // = "largest offset", registers start at 0).  Settled here, once per line, so the row building below stays as it is.
        const uint32_t* fw = reinterpret_cast<const uint32_t*>(smem + foldOff);
        TdfaReg* rw = reinterpret_cast<TdfaReg*>(smem + regsBase) + tdfaRegLane<TdfaReg>(tid);
        const uint32_t nWords = __builtin_amdgcn_readfirstlane(fw[0]);
        for (uint32_t i0 = 0; i0 < nWords; i0 += 64) {
            const uint32_t fwv = (i0 + lane < nWords) ? fw[1 + i0 + lane] : 0xFFFFFF00u;  // (lane i holds word i0 + i)
            const uint32_t cnt = nWords - i0 < 64 ? nWords - i0 : 64;
            for (uint32_t j0 = 0; j0 < cnt; j0 += 4) {
                uint32_t w[4];
                TdfaReg both[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // four set registers per round trip
                    w[k] = uint32_t(__builtin_amdgcn_readlane(int(fwv), int((j0 + k) & 63)));
                    both[k] = rw[(w[k] & 0xFFu) * BLOCK];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (j0 + k >= cnt) break;
                    if (!__any(both[k] != 0)) continue;  // no line of the wave took such a transition (the usual case)
                    // (a set register is never the member of another set: the four reads above stay valid)
#pragma unroll
                    for (int m = 1; m < 4; ++m) {
                        const uint32_t r = (w[k] >> (8 * m)) & 0xFFu;
                        if (r != 0xFFu) {
                            const TdfaReg own = rw[r * BLOCK];
                            rw[r * BLOCK] = both[k] > own ? both[k] : own;
                        }
                    }
                }
            }
        }
    }
    constexpr uint32_t kTileWords = 1024;  // 64 rows x 64 bytes: the smaller of the two tile layouts
    const bool viaTile = !permuted && nOut != 0 && nOut <= kTileWords && __all(live);
    // Lines of one format end in the same accepting state: then the slot -> register map is the same for the whole wave
    // and the row is built without a per-slot, per-lane map lookup and its branches.
    const uint32_t fid0 = __builtin_amdgcn_readfirstlane(fid);
    const bool sameMap = __all(fid == fid0) && fid0 != 0xFFFFu;
    // The usual wave (one format, at most kRowRegs slots, at most 64 derive words): every lane reads the registers behind its nOut
    // slots ONCE, into VGPRs -- the walk's are dead by now --, and the derive words are applied to the slot map (a derived slot
    // reads as its source register + the sum of the deltas: wave-uniform) instead of to every lane's registers in LDS.  It used
    // to be 24 register reads for 20 slots in each of the two passes, behind a read-add-write chain per derive word.
    constexpr uint32_t kRowRegs = 24;
    // one-stamp pair tables: a register that is only ever stamped one byte behind another one lost its own stamps and reads as that
    // one + delta (device_tables.h TP_OFF_DERIVE; in table order: every source is settled before it is used)
    uint32_t nDerive = 0;
    const uint32_t* deriveWords = nullptr;
    if constexpr ((LAB & kLabPairOne) != 0) {
        const uint32_t* ph = reinterpret_cast<const uint32_t*>(smem + hdr[TD_OFF_PAIR]);
        const uint32_t dOff = ph[TP_OFF_DERIVE];
        if (dOff) {
            deriveWords = reinterpret_cast<const uint32_t*>(smem + dOff) + 1;
            nDerive = __builtin_amdgcn_readfirstlane(deriveWords[-1]);
        }
    }
    const bool rowInRegs = viaTile && sameMap && nOut <= kRowRegs && nDerive <= 64;
    if (!rowInRegs && nDerive != 0) {  // every other path reads the registers from LDS: the words are applied there, in table order
        TdfaReg* rw = reinterpret_cast<TdfaReg*>(smem + regsBase) + tdfaRegLane<TdfaReg>(tid);
        for (uint32_t i = 0; i < nDerive; ++i) {
            const uint32_t w = __builtin_amdgcn_readfirstlane(deriveWords[i]);
            rw[(w & 0xFFu) * BLOCK] = TdfaReg(rw[((w >> 8) & 0xFFu) * BLOCK] + TdfaReg(w >> 16));
        }
    }
    auto slotValue = [&](uint32_t s) -> int32_t {
        int32_t val = -1;
        if (matched && s < nSlots) {
            const uint32_t m = finalMap[fid * nSlots + s];
            if (m == TD_REG_POS) val = int32_t(L + from);
            else if (m != TD_REG_NONE) val = int32_t(regs[m * BLOCK + rl] + from);
        }
        return val;
    };
    if (viaTile) {
        int32_t* tile = reinterpret_cast<int32_t*>(smem + tileAddr);
        uint32_t rowsPerPass = kTileWords / nOut;
        if (rowsPerPass > 64) rowsPerPass = 64;
        if (rowsPerPass > 1) rowsPerPass &= ~1u;  // even: every pass starts on a 16-byte boundary of the capture table (nOut is even)
        int32_t* gout = caps + size_t(line - lane) * nOut;  // (lines of the wave are consecutive: line - lane = lane 0's)
        const int32_t end = int32_t(L + from);
        int32_t rowv[kRowRegs];
        if (rowInRegs) {
            // lane i resolves slot i: its register, followed back through the derive words (last word first: a word's source is
            // settled by the words before it), and the deltas met on the way
            const uint8_t* map = finalMap + fid0 * nSlots;
            const uint32_t mapv = (lane < nSlots && lane < nOut) ? uint32_t(map[lane]) : uint32_t(TD_REG_NONE);
            const uint32_t dwv = lane < nDerive ? deriveWords[lane] : 0u;  // (lane i holds derive word i)
            uint32_t root = mapv, dsum = 0;
            for (uint32_t i = nDerive; i-- > 0;) {
                const uint32_t w = uint32_t(__builtin_amdgcn_readlane(int(dwv), int(i)));
                const bool hit = root == (w & 0xFFu);  // (TD_REG_POS / TD_REG_NONE are no register: never a word's target)
                root = hit ? (w >> 8) & 0xFFu : root;
                dsum += hit ? w >> 16 : 0u;
            }
#pragma unroll
            for (int k = 0; k < int(kRowRegs); k += 2) {  // (nOut is even; wave-uniform: no read past the row's slots)
                if (uint32_t(k) < nOut) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t m = uint32_t(__builtin_amdgcn_readlane(int(root), k + h));
                        const uint32_t d = uint32_t(__builtin_amdgcn_readlane(int(dsum), k + h));
                        const uint32_t r = m < TD_REG_NONE ? m : 0u;
                        const int32_t reg = int32_t(TdfaReg(regs[r * BLOCK + rl] + TdfaReg(d)) + from);
                        int32_t val = m == TD_REG_POS ? end : reg;
                        val = m == TD_REG_NONE ? -1 : val;
                        rowv[k + h] = state != 0 ? val : -1;
                    }
                }
            }
        }
        for (uint32_t p0 = 0; p0 < 64; p0 += rowsPerPass) {
            tdfaWaveLdsSync();
            const bool inPass = lane >= p0 && lane - p0 < rowsPerPass;
            int32_t* row = tile + (inPass ? lane - p0 : 0u) * nOut;
            if (rowInRegs) {
                if (inPass) {
#pragma unroll
                    for (int k = 0; k < int(kRowRegs); k += 2) {
                        if (uint32_t(k) < nOut) {
                            row[k] = rowv[k];
                            row[k + 1] = rowv[k + 1];
                        }
                    }
                }
            } else if (sameMap) {
                const uint8_t* map = finalMap + fid0 * nSlots;
                for (uint32_t s0 = 0; s0 < nOut; s0 += 64) {  // (one trip unless the pattern has more than 32 groups)
                    const uint32_t sl = s0 + lane;
                    const uint32_t mapv = (sl < nSlots && sl < nOut) ? uint32_t(map[sl]) : uint32_t(TD_REG_NONE);  // lane i: slot s0 + i
                    const uint32_t cnt = nOut - s0 < 64 ? nOut - s0 : 64;
                    for (uint32_t k0 = 0; k0 < cnt; k0 += 8) {
                        int32_t v[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) {  // (m is wave-uniform; the register read is issued whatever m says)
                            const uint32_t m = uint32_t(__builtin_amdgcn_readlane(int(mapv), int((k0 + k) & 63)));
                            const uint32_t r = m < TD_REG_NONE ? m : 0u;
                            const int32_t reg = int32_t(regs[r * BLOCK + rl] + from);
                            int32_t val = m == TD_REG_POS ? end : reg;
                            val = m == TD_REG_NONE ? -1 : val;
                            v[k] = state != 0 ? val : -1;
                        }
                        if (inPass) {
#pragma unroll
                            for (int k = 0; k < 8; ++k)
                                if (k0 + k < cnt) row[s0 + k0 + k] = v[k];
                        }
                    }
                }
            } else if (inPass) {
#pragma unroll 4
                for (uint32_t s = 0; s < nOut; ++s) row[s] = slotValue(s);
            }
            tdfaWaveLdsSync();
            const uint32_t rows = 64 - p0 < rowsPerPass ? 64 - p0 : rowsPerPass;
            const uint32_t total = rows * nOut;
            int32_t* g = gout + size_t(p0) * nOut;
            if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0 && (total & 3u) == 0) {  // (wave-uniform)
                typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
                const uint32_t nq = total / 4;  // <= 256: at most four 16-byte pieces per lane
                i32x4 q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t at = lane + 64u * uint32_t(i);
                    if (at < nq) q[i] = *reinterpret_cast<const i32x4 __attribute__((address_space(3)))*>(tileAddr + at * 16u);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t at = lane + 64u * uint32_t(i);
                    // (non-temporal: the capture table is written once and not read again by this kernel; round 3 lab: -1 %)
                    if (at < nq) __builtin_nontemporal_store(q[i], reinterpret_cast<i32x4*>(g) + at);
                }
            } else {
                for (uint32_t d = lane; d < total; d += 64) g[d] = tile[d];
            }
        }
    } else if (live) {
        int32_t* out = caps + size_t(line) * nOut;
        for (uint32_t s = 0; s < nOut; ++s) out[s] = slotValue(s);
    }
    if (live) status[line] = matched ? LC_MATCH : LC_NOMATCH;
}

// Completion signal of a launch whose caller polls host memory instead of asking the runtime (gpu_runtime.hip, the zero-copy
// host path): every workgroup publishes its results system-wide and counts itself; the last one resets the counter and stores
// the launch's sequence number into the caller's pinned flag word.  doneFlag == nullptr: nothing to do.
__device__ __forceinline__ void tdfaSignalDone(uint32_t* doneCounter, uint32_t* doneFlag, uint32_t doneSeq) {
    if (!doneFlag) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(doneCounter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(doneCounter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(doneFlag, doneSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Byte-PAIR stepping (device_tables.h TP_*): the state chain -- the only serial dependency, one LDS round trip per link --
// has one link per TWO bytes: t = pair32[(t & 0xFFFF) + cmapA[byte 2k] + cmap8[byte 2k+1]].  The entry also names the
// register each of the two bytes stamps.  Where the pair table sits in the staged blob:
struct TdfaPairInfo {
    uint32_t base, rowBytes, cmapA, idA;
};
typedef const uint16_t __attribute__((address_space(3))) * LdsHalfPtr;
