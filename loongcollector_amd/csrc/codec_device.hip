// codec_device.hip -- the engine level of the field codecs (include/codec/lc_codec.h): the launches of codec_kernel.hpp around the scan of
// scan64_kernel.hpp, the calling thread's scratch, and the host entry's trip through a runner thread's pinned staging.  The handle and
// everything the Go plugins do around the rewrite live in processor_codec_gpu.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/codec/lc_codec.h"
#include "codec_kernel.hpp"
#include "packed_trip.hpp"
#include "processor_codec_gpu.hpp"
#include "scan64_kernel.hpp"

namespace {
// lanes per value of the two write passes (-DLC_CODEC_LANES=.. builds a variant for tools/codec_bench.py --lib)
#ifdef LC_CODEC_LANES
constexpr uint32_t kWriteLanes = LC_CODEC_LANES;
#else
constexpr uint32_t kWriteLanes = 16;
#endif

// per runner thread: the scratch of a call (the CLEAN bytes, the scan's tile sums, pinned words), and the host entry's stream and
// staging; grow-only
struct CodecThread : TripThread<CodecThread> {
    TripBuf hIn, hOut, dIn, dOut, dFlags, dErrOff, dOutOff, dOutLen;  // the host entry's
    TripBuf dClean, dTileSums, hWord;                                // every call's
    int scratchDevice = -1;
    CodecThread() : TripThread(true) { hIn.pinned = hOut.pinned = hWord.pinned = true; }
    ~CodecThread() {
        if (lcRuntimeUsable() && (stream || scratchDevice >= 0)) release();
    }
    void releaseScratch() {
        for (TripBuf* b : {&dClean, &dTileSums, &hWord}) b->release();
        scratchDevice = -1;
    }
    void release() {
        releaseWith({&hIn, &hOut, &dIn, &dOut, &dFlags, &dErrOff, &dOutOff, &dOutLen});
        releaseScratch();
    }
};
thread_local CodecThread tlsCodec;

inline uint32_t blocksFor(uint64_t items, uint32_t perBlock) { return uint32_t((items + perBlock - 1) / perBlock); }

// lengths or size pass, scan, (the total comes to the host,) write.  offEnd: d_off[n] when the caller knows it, UINT64_MAX when it must
// be read.  room(total, &rc, &cap) -> where the output bytes go and how many fit there, or nullptr with rc set.
template <class Room>
int applyOnStream(const CodecConfig& cfg, int dev, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint64_t offEnd, uint8_t* d_flags,
                  uint32_t* d_err_off, uint64_t* d_out_off, uint32_t* d_out_len, Room room, uint64_t* needed, hipStream_t st) {
    CodecThread& T = tlsCodec;
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
            lcSetLastError("lc_codec_apply_device: d_off does not ascend");
            return LC_ERR_ARG;
        }
        offEnd = hWord[1];
    }
    if (offEnd >= (1ull << 31)) {
        lcSetLastError("lc_codec_apply: a batch of 2 GiB or more");
        return LC_ERR_ARG;
    }
    const uint32_t perValueBlocks = blocksFor(uint64_t(n) + 1, lccodec::kBlock);
    if (cfg.op == kCodecDecode) {
        LC_HIP_TRY(T.dClean.ensure(tripRoundUp(n, 64)));
        lcNoteKernel("b64_decode_size_kernel");
        hipLaunchKernelGGL(lccodec::b64_decode_size_kernel, dim3(perValueBlocks), dim3(lccodec::kBlock), 0, st, d_data, d_off, n, d_flags, d_err_off, d_out_off,
                           d_out_len, static_cast<uint8_t*>(T.dClean.p));
    } else {
        lcNoteKernel("codec_len_kernel");
        hipLaunchKernelGGL(lccodec::codec_len_kernel, dim3(perValueBlocks), dim3(lccodec::kBlock), 0, st, cfg.op, d_off, n, d_flags, d_out_off, d_out_len);
    }
    LC_HIP_TRY(hipGetLastError());
    uint64_t total = 32ull * n;  // MD5: a fixed stride, no scan
    if (cfg.op != kCodecMd5) {
        LC_HIP_TRY(T.dTileSums.ensure(lcscan::tileSumBytes(uint64_t(n) + 1)));
        lcNoteKernel("scan64_kernel");
        LC_HIP_TRY(lcscan::exclusiveScan(d_out_off, n + 1, static_cast<uint64_t*>(T.dTileSums.p), st));
        LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord) + 2, d_out_off + n, 8, hipMemcpyDeviceToHost, st));
    }
    LC_HIP_TRY(hipStreamSynchronize(st));
    if (cfg.op != kCodecMd5) total = uint64_t(hWord[2]) | uint64_t(hWord[3]) << 32;
    if (needed) *needed = total;
    if (total == 0) return LC_OK;  // nothing but empty values and errors
    int rc = LC_OK;
    uint64_t cap = 0;
    uint8_t* d_out = room(total, &rc, &cap);
    if (!d_out) return rc;
    const uint32_t writeBlocks = blocksFor(uint64_t(n) * kWriteLanes, lccodec::kBlock);
    if (cfg.op == kCodecEncode) {
        lcNoteKernel("b64_encode_kernel");
        hipLaunchKernelGGL(lccodec::b64_encode_kernel<kWriteLanes>, dim3(writeBlocks), dim3(lccodec::kBlock), 0, st, d_data, d_off, n,
                           static_cast<const uint64_t*>(d_out_off), d_out, cap);
    } else if (cfg.op == kCodecDecode) {
        lcNoteKernel("b64_decode_write_kernel");
        hipLaunchKernelGGL(lccodec::b64_decode_write_kernel<kWriteLanes>, dim3(writeBlocks), dim3(lccodec::kBlock), 0, st, d_data, d_off, n,
                           static_cast<const uint8_t*>(d_flags), static_cast<const uint8_t*>(T.dClean.p), static_cast<const uint64_t*>(d_out_off),
                           static_cast<const uint32_t*>(d_out_len), d_out, cap);
    } else {
        lcNoteKernel("md5_field_kernel");
        hipLaunchKernelGGL(lccodec::md5_field_kernel, dim3(blocksFor(n, lccodec::kBlock)), dim3(lccodec::kBlock), 0, st, d_data, d_off, n, d_out, cap);
    }
    LC_HIP_TRY(hipGetLastError());
    // (the CLEAN bytes the kernel reads are the calling thread's: they must not be reused by the thread's next call before it is through)
    LC_HIP_TRY(hipStreamSynchronize(st));
    return LC_OK;
}
}  // namespace

extern "C" void lc_codec_thread_release(void) { tlsCodec.release(); }

extern "C" int lc_codec_apply_device(const lc_codec_t* p, const uint8_t* d_data, const uint32_t* d_off, uint32_t n, uint8_t* d_flags, uint32_t* d_err_off,
                                     uint64_t* d_out_off, uint32_t* d_out_len, uint8_t* d_out, uint64_t out_cap, uint64_t* needed, void* stream) {
    if (needed) *needed = 0;
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_flags || !d_out_off || !d_out_len || (!d_out && out_cap) || (reinterpret_cast<uintptr_t>(d_out_off) & 7) ||
        (reinterpret_cast<uintptr_t>(d_off) & 3) || (reinterpret_cast<uintptr_t>(d_out_len) & 3) || (reinterpret_cast<uintptr_t>(d_err_off) & 3) ||
        (reinterpret_cast<uintptr_t>(d_out) & 15) || n >= (1u << 31))
        return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the field codecs have no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return applyOnStream(lcCodecConfig(p), dev, d_data, d_off, n, UINT64_MAX, d_flags, d_err_off, d_out_off, d_out_len,
                         [&](uint64_t total, int* rc, uint64_t* cap) -> uint8_t* {
                             *cap = out_cap;  // (the kernel holds the total against it once more: too small, and not one byte is stored)
                             if (total <= out_cap) return d_out;
                             lcSetLastError("lc_codec_apply_device: the output needs " + std::to_string(total) + " bytes");
                             *rc = LC_ERR_OVERFLOW;
                             return nullptr;
                         },
                         needed, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
constexpr size_t kChunkBytes = 32u << 20;   // payload bytes per trip: 4/3 of it and 19 bytes of rounding per value stay below 256 MiB
constexpr uint32_t kChunkLines = 1u << 18;  // and at most this many values (32 bytes of digest each)
constexpr size_t kChunkResultBytes = 64u << 20;
constexpr size_t kLineResultBytes = 8 + 4 + 4 + 1;  // out_off, out_len, err_off, flags
std::atomic<size_t> gTripBytes{0};
std::atomic<uint64_t> gTrips{0};
}  // namespace

extern "C" uint64_t lc_codec_set_trip_bytes(size_t bytes) {
    gTripBytes.store(bytes);
    return gTrips.exchange(0);
}

extern "C" int lc_codec_apply_host(const lc_codec_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint32_t* err_off,
                                   uint64_t* out_off, uint32_t* out_len, uint8_t** out) {
    if (out) *out = nullptr;
    if (!p || !out || !out_off) return LC_ERR_ARG;
    out_off[0] = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !flags || !out_len) return LC_ERR_ARG;
    CodecThread& T = tlsCodec;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the field codecs have no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    std::vector<uint8_t> bytes;
    const size_t tripBytes = gTripBytes.load() ? gTripBytes.load() : kChunkBytes;
    // the input half of the packed trip alone (packed_trip.hpp): the result sizes are known only once applyOnStream is through
    const PackedTripSpec spec{"lc_codec_apply_host", "value", kChunkLines, tripBytes, kLineResultBytes, kChunkResultBytes, nullptr};
    PackedChunk c;
    while (c.next < n) {
        if (const int rc = packedTripPlan(T, spec, len, n, &c); rc != LC_OK) return rc;
        const uint32_t next = c.next, cnt = c.cnt;
        ++gTrips;
        LC_HIP_TRY(T.dFlags.ensure(tripRoundUp(cnt, 64)));
        LC_HIP_TRY(T.dErrOff.ensure(size_t(cnt) * 4));
        LC_HIP_TRY(T.dOutLen.ensure(size_t(cnt) * 4));
        LC_HIP_TRY(T.dOutOff.ensure((size_t(cnt) + 1) * 8));
        if (const int rc = packedTripUpload(T, lines, len, c); rc != LC_OK) return rc;
        uint8_t* dIn = c.dIn;
        uint64_t needed = 0;
        int rc = applyOnStream(lcCodecConfig(p), dev, dIn, reinterpret_cast<const uint32_t*>(dIn + c.in.offAt), cnt, c.bytes, static_cast<uint8_t*>(T.dFlags.p),
                               static_cast<uint32_t*>(T.dErrOff.p), static_cast<uint64_t*>(T.dOutOff.p), static_cast<uint32_t*>(T.dOutLen.p),
                               [&](uint64_t totalBytes, int* rcRoom, uint64_t* cap) -> uint8_t* {
                                   const hipError_t e = T.dOut.ensure(size_t(totalBytes));
                                   *cap = T.dOut.cap;
                                   if (e == hipSuccess) return static_cast<uint8_t*>(T.dOut.p);
                                   *rcRoom = lcHipFail(e, "T.dOut.ensure(output bytes)");
                                   return nullptr;
                               },
                               &needed, T.stream);
        // the results come down: out_off, out_len, err_off, flags, then the bytes -- one trip's end for all five
        const size_t lenAt = (size_t(cnt) + 1) * 8, errAt = lenAt + size_t(cnt) * 4, flagsAt = errAt + size_t(cnt) * 4;
        const size_t bytesAt = tripRoundUp(flagsAt + cnt, 64);
        if (rc == LC_OK) {
            const hipError_t e = T.hOut.ensure(bytesAt + size_t(needed));
            if (e != hipSuccess) rc = lcHipFail(e, "T.hOut.ensure(results)");
        }
        uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
        if (rc == LC_OK) {
            hipError_t e = hipMemcpyAsync(hOut, T.dOutOff.p, lenAt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hOut + lenAt, T.dOutLen.p, size_t(cnt) * 4, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hOut + errAt, T.dErrOff.p, size_t(cnt) * 4, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hOut + flagsAt, T.dFlags.p, cnt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess && needed) e = hipMemcpyAsync(hOut + bytesAt, T.dOut.p, size_t(needed), hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(codec results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint64_t base = bytes.size();  // (a multiple of 16, as every trip's total is)
        const uint64_t* chunkOff = reinterpret_cast<const uint64_t*>(hOut);
        const uint32_t* chunkErr = reinterpret_cast<const uint32_t*>(hOut + errAt);
        for (uint32_t i = 0; i <= cnt; ++i) out_off[next + i] = base + chunkOff[i];
        std::memcpy(out_len + next, hOut + lenAt, size_t(cnt) * 4);
        std::memcpy(flags + next, hOut + flagsAt, cnt);
        if (err_off)
            for (uint32_t i = 0; i < cnt; ++i)
                if (flags[next + i] & LC_CODEC_ERROR) err_off[next + i] = chunkErr[i];
        bytes.insert(bytes.end(), hOut + bytesAt, hOut + bytesAt + needed);
        c.advance(len);
    }
    if (!bytes.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(bytes.size()));
        if (!*out) {
            lcSetLastError("lc_codec_apply_host: out of memory for " + std::to_string(bytes.size()) + " output bytes");
            return LC_ERR_OVERFLOW;
        }
        std::memcpy(*out, bytes.data(), bytes.size());
    }
    return LC_OK;
}
