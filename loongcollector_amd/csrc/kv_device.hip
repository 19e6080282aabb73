// kv_device.hip -- the engine level of the key-value splitter (include/kvsplit/lc_kvsplit.h): the launch of kv_split_kernel (kv_kernel.hpp)
// and the host entry's trip through a runner thread's pinned staging.  The handle and everything the Go plugin does around the split
// live in processor_split_key_value_gpu.cpp.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/kvsplit/lc_kvsplit.h"
#include "kv_kernel.hpp"
#include "packed_trip.hpp"
#include "processor_split_key_value_gpu.hpp"

static int launchSplit(const KvConfig& cfg, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_npairs,
                       int32_t* d_pairs, hipStream_t st) {
    const dim3 grid((n + lckv::kBlock - 1) / lckv::kBlock), block(lckv::kBlock);
    lcNoteKernel("kv_split_kernel");
    lckv::KvNeedleWords words;
    std::memcpy(words.w, cfg.delim, lckv::kNeedleBytes);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, words, cfg.delimLen, cfg.sepLen, cfg.quoteLen, d_data, d_off, n, W, d_status, d_npairs, d_pairs);
    };
    if (cfg.quoteLen > 1) launch(lckv::kv_split_kernel<kKvQuoteLong>);
    else if (cfg.quoteLen == 1) launch(lckv::kv_split_kernel<kKvQuoteOne>);
    else launch(lckv::kv_split_kernel<kKvQuoteNone>);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// splitKeyValue (key_value_splitter.go:99-143) for n values at once
extern "C" int lc_kvsplit_device(const lc_kvsplit_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status,
                                 uint32_t* d_npairs, int32_t* d_pairs, void* stream) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_status || !d_npairs || (W && !d_pairs)) return LC_ERR_ARG;
    // aligned for the stores the kernel makes (a row: one 16-byte vector)
    if ((reinterpret_cast<uintptr_t>(d_npairs) & 3u) || (W && (reinterpret_cast<uintptr_t>(d_pairs) & 15u))) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the key-value splitter has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchSplit(lcKvConfig(p), d_data, d_off, n, W, d_status, d_npairs, d_pairs, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
thread_local PackedThread<struct KvTag> tlsKv;
}  // namespace

extern "C" void lc_kvsplit_thread_release(void) { tlsKv.release(); }

extern "C" int lc_kvsplit_host(const lc_kvsplit_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status,
                               uint32_t* npairs, int32_t* pairs) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !npairs || (W && !pairs)) return LC_ERR_ARG;
    auto& T = tlsKv;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the key-value splitter has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t valueRowBytes = size_t(W) * 16;
    // a chunk: 32 MiB of payload, 2^18 values, 64 MiB of rows; down come the rows, the counts and the status bytes
    const PackedTripSpec spec{"lc_kvsplit_host", "value", 1u << 18, 32u << 20, valueRowBytes + 4 + 1, 64u << 20, "hipMemcpyAsync(key-value results)"};
    enum { kRows, kNpairs, kStatus };
    const KvConfig& cfg = lcKvConfig(p);
    return packedTrip(
        T, spec, lines, len, n, {valueRowBytes, 4, 1},
        [&](const PackedChunk& c) {
            return launchSplit(cfg, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, W, c.dResult<uint8_t>(kStatus),
                               c.dResult<uint32_t>(kNpairs), c.dResult<int32_t>(kRows), T.stream);
        },
        [&](PackedChunk& c) {
            const uint32_t* np = reinterpret_cast<const uint32_t*>(c.hResult(kNpairs, 4));
            const uint8_t* hRows = c.hResult(kRows, valueRowBytes);
            for (uint32_t i = 0; W && i < c.cnt; ++i) {  // only what the kernel wrote: the caller's array keeps what it held behind it
                const uint32_t k = np[i] < W ? np[i] : W;
                if (k) std::memcpy(pairs + (size_t(c.next) + i) * W * 4, hRows + size_t(i) * valueRowBytes, size_t(k) * 16);
            }
            std::memcpy(npairs + c.next, np, size_t(c.cnt) * 4);
            std::memcpy(status + c.next, c.hResult(kStatus, 1), c.cnt);
            return LC_OK;
        });
}
