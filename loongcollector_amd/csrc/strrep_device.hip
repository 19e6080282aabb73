// strrep_device.hip -- the engine level of the string-replace processor (include/strrep/lc_strrep.h): the launches of strrep_kernel.hpp
// around the scan of scan64_kernel.hpp, the calling thread's scratch, and the host entry's trip through a runner thread's pinned staging.
// The handle and everything the Go plugin does around the rewrite live in processor_string_replace_gpu.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/strrep/lc_strrep.h"
#include "packed_trip.hpp"
#include "processor_string_replace_gpu.hpp"
#include "scan64_kernel.hpp"
#include "strrep_kernel.hpp"

namespace {
// lanes per value of the write pass (DESIGN.md section 5.21 has the figures of 4 to 64; -DLC_STRREP_LANES=.. builds a variant for
// tools/string_replace_bench.py --lib)
#ifdef LC_STRREP_LANES
constexpr uint32_t kWriteLanes = LC_STRREP_LANES;
#else
constexpr uint32_t kWriteLanes = 16;
#endif

// per runner thread: the scratch of a call (records, the scan's tile sums, two pinned words), and the host entry's stream and staging;
// grow-only
struct StrrepThread : TripThread<StrrepThread> {
    TripBuf hIn, hOut, dIn, dOut, dFlags, dOutOff;  // the host entry's
    TripBuf dRecords, dTileSums, hWord;             // every call's
    int scratchDevice = -1;
    StrrepThread() : TripThread(true) { hIn.pinned = hOut.pinned = hWord.pinned = true; }
    ~StrrepThread() {
        if (lcRuntimeUsable() && (stream || scratchDevice >= 0)) release();
    }
    void releaseScratch() {
        for (TripBuf* b : {&dRecords, &dTileSums, &hWord}) b->release();
        scratchDevice = -1;
    }
    void release() {
        releaseWith({&hIn, &hOut, &dIn, &dOut, &dFlags, &dOutOff});
        releaseScratch();
    }
};
thread_local StrrepThread tlsStrrep;

inline uint32_t blocksFor(uint64_t items, uint32_t perBlock) { return uint32_t((items + perBlock - 1) / perBlock); }

// size, scan, (the total comes to the host,) write.  offEnd: d_off[n] when the caller knows it, UINT64_MAX when it must be read.
// room(total, &rc, &cap) -> where the output bytes go and how many fit there, or nullptr with rc set.
template <class Room>
int applyOnStream(const StrrepConfig& cfg, int dev, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint64_t offEnd, uint8_t* d_flags,
                  uint64_t* d_out_off, Room room, uint64_t* needed, hipStream_t st) {
    StrrepThread& T = tlsStrrep;
    if (T.scratchDevice != dev) {
        if (T.scratchDevice >= 0) T.releaseScratch();
        T.scratchDevice = dev;
        lcRegisterExitHook();
    }
    LC_HIP_TRY(T.hWord.ensure(64));
    volatile uint32_t* hWord = static_cast<volatile uint32_t*>(T.hWord.p);
    if (offEnd == UINT64_MAX) {
        LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord), d_off, 4, hipMemcpyDeviceToHost, st));
        LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord) + 1, d_off + n, 4, hipMemcpyDeviceToHost, st));
        LC_HIP_TRY(hipStreamSynchronize(st));
        if (hWord[0] > hWord[1]) {
            lcSetLastError("lc_strrep_apply_device: d_off does not ascend");
            return LC_ERR_ARG;
        }
        offEnd = hWord[1];
    }
    if (offEnd >= (1ull << 31)) {
        lcSetLastError("lc_strrep_apply: a batch of 2 GiB or more");
        return LC_ERR_ARG;
    }
    const size_t slots = size_t((offEnd + 63) >> 6) + n + 2;
    LC_HIP_TRY(T.dRecords.ensure(slots * 16));
    LC_HIP_TRY(T.dTileSums.ensure(lcscan::tileSumBytes(uint64_t(n) + 1)));
    lcNoteKernel("strrep_size_kernel");
    hipLaunchKernelGGL(lcstrrep::strrep_size_kernel, dim3(blocksFor(uint64_t(n) + 1, lcstrrep::kBlock)), dim3(lcstrrep::kBlock), 0, st, cfg, d_data, d_off, n,
                       d_flags, d_out_off, static_cast<lcwave::u32x4*>(T.dRecords.p));
    LC_HIP_TRY(hipGetLastError());
    lcNoteKernel("scan64_kernel");
    LC_HIP_TRY(lcscan::exclusiveScan(d_out_off, n + 1, static_cast<uint64_t*>(T.dTileSums.p), st));
    LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord) + 2, d_out_off + n, 8, hipMemcpyDeviceToHost, st));
    LC_HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = uint64_t(hWord[2]) | uint64_t(hWord[3]) << 32;
    if (needed) *needed = total;
    if (total == 0) return LC_OK;  // nothing changed, or only to empty values
    int rc = LC_OK;
    uint64_t cap = 0;
    uint8_t* d_out = room(total, &rc, &cap);
    if (!d_out) return rc;
    lcNoteKernel("strrep_write_kernel");
    hipLaunchKernelGGL(lcstrrep::strrep_write_kernel<kWriteLanes>, dim3(blocksFor(uint64_t(n) * kWriteLanes, lcstrrep::kBlock)), dim3(lcstrrep::kBlock), 0, st,
                       cfg, d_data, d_off, n, static_cast<const uint8_t*>(d_flags), static_cast<const uint64_t*>(d_out_off),
                       static_cast<const uint32_t*>(T.dRecords.p), d_out, cap);
    LC_HIP_TRY(hipGetLastError());
    // (the records the kernel reads are the calling thread's: they must not be reused by the thread's next call before it is through)
    LC_HIP_TRY(hipStreamSynchronize(st));
    return LC_OK;
}
}  // namespace

extern "C" void lc_strrep_thread_release(void) { tlsStrrep.release(); }

extern "C" int lc_strrep_apply_device(const lc_strrep_t* p, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint8_t* d_flags, uint64_t* d_out_off,
                                      uint8_t* d_out, uint64_t out_cap, uint64_t* needed, void* stream) {
    if (needed) *needed = 0;
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_flags || !d_out_off || (!d_out && out_cap) || (reinterpret_cast<uintptr_t>(d_out_off) & 7) ||
        (reinterpret_cast<uintptr_t>(d_off) & 3) || n >= (1u << 31))
        return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the string-replace processor has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return applyOnStream(lcStrrepConfig(p), dev, d_data, d_off, n, UINT64_MAX, d_flags, d_out_off,
                         [&](uint64_t total, int* rc, uint64_t* cap) -> uint8_t* {
                             *cap = out_cap;  // (the kernel holds the total against it once more: too small, and not one byte is stored)
                             if (total <= out_cap) return d_out;
                             lcSetLastError("lc_strrep_apply_device: the output needs " + std::to_string(total) + " bytes");
                             *rc = LC_ERR_OVERFLOW;
                             return nullptr;
                         },
                         needed, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
constexpr size_t kChunkBytes = 32u << 20;   // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;  // and at most this many values
constexpr size_t kChunkResultBytes = 64u << 20;
constexpr size_t kLineResultBytes = 8 + 1;  // out_off, flags
constexpr size_t kChunkOutputBytes = 256u << 20;  // what a trip's new bytes may take at the worst

// the payload of a trip, cut so that its output stays below kChunkOutputBytes whatever the values hold: const grows a value by at most
// len(ReplaceString) / len(Match), the unquote by at most three (a single value above the cut still travels alone)
size_t chunkPayloadBytes(const StrrepConfig& cfg) {
    const size_t growth = cfg.method == kStrrepConst ? (cfg.replLen + cfg.matchLen - 1) / cfg.matchLen : 3;
    const size_t fits = kChunkOutputBytes / (growth ? growth : 1);
    return fits < kChunkBytes ? fits : kChunkBytes;
}
}  // namespace

extern "C" int lc_strrep_apply_host(const lc_strrep_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint64_t* out_off,
                                    uint8_t** out) {
    if (out) *out = nullptr;
    if (!p || !out || !out_off) return LC_ERR_ARG;
    out_off[0] = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !flags) return LC_ERR_ARG;
    StrrepThread& T = tlsStrrep;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the string-replace processor has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    std::vector<uint8_t> bytes;
    // the input half of the packed trip alone (packed_trip.hpp): the result sizes are known only once applyOnStream is through
    const PackedTripSpec spec{"lc_strrep_apply_host", "value", kChunkLines, chunkPayloadBytes(lcStrrepConfig(p)), kLineResultBytes, kChunkResultBytes, nullptr};
    PackedChunk c;
    while (c.next < n) {
        if (const int rc = packedTripPlan(T, spec, len, n, &c); rc != LC_OK) return rc;
        const uint32_t next = c.next, cnt = c.cnt;
        LC_HIP_TRY(T.dFlags.ensure(tripRoundUp(cnt, 64)));
        LC_HIP_TRY(T.dOutOff.ensure((size_t(cnt) + 1) * 8));
        if (const int rc = packedTripUpload(T, lines, len, c); rc != LC_OK) return rc;
        uint8_t* dIn = c.dIn;
        uint64_t needed = 0;
        int rc = applyOnStream(lcStrrepConfig(p), dev, dIn, reinterpret_cast<const uint32_t*>(dIn + c.in.offAt), cnt, c.bytes, static_cast<uint8_t*>(T.dFlags.p),
                               static_cast<uint64_t*>(T.dOutOff.p),
                               [&](uint64_t totalBytes, int* rcRoom, uint64_t* cap) -> uint8_t* {
                                   const hipError_t e = T.dOut.ensure(size_t(totalBytes));
                                   *cap = T.dOut.cap;
                                   if (e == hipSuccess) return static_cast<uint8_t*>(T.dOut.p);
                                   *rcRoom = lcHipFail(e, "T.dOut.ensure(output bytes)");
                                   return nullptr;
                               },
                               &needed, T.stream);
        // the results come down: out_off, flags, then the bytes -- one trip's end for all three
        const size_t flagsAt = (size_t(cnt) + 1) * 8;
        const size_t bytesAt = tripRoundUp(flagsAt + cnt, 64);
        if (rc == LC_OK) {
            const hipError_t e = T.hOut.ensure(bytesAt + size_t(needed));
            if (e != hipSuccess) rc = lcHipFail(e, "T.hOut.ensure(results)");
        }
        uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
        if (rc == LC_OK) {
            hipError_t e = hipMemcpyAsync(hOut, T.dOutOff.p, flagsAt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hOut + flagsAt, T.dFlags.p, cnt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess && needed) e = hipMemcpyAsync(hOut + bytesAt, T.dOut.p, size_t(needed), hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(string-replace results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint64_t base = bytes.size();
        const uint64_t* chunkOff = reinterpret_cast<const uint64_t*>(hOut);
        for (uint32_t i = 0; i <= cnt; ++i) out_off[next + i] = base + chunkOff[i];
        std::memcpy(flags + next, hOut + flagsAt, cnt);
        bytes.insert(bytes.end(), hOut + bytesAt, hOut + bytesAt + needed);
        c.advance(len);
    }
    if (!bytes.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(bytes.size()));
        if (!*out) {
            lcSetLastError("lc_strrep_apply_host: out of memory for " + std::to_string(bytes.size()) + " output bytes");
            return LC_ERR_OVERFLOW;
        }
        std::memcpy(*out, bytes.data(), bytes.size());
    }
    return LC_OK;
}
