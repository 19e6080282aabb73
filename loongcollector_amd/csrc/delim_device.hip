// delim_device.hip -- the engine level of the delimiter parser (include/lc_delimiter.h): the handle, the launch of
// delim_split_kernel (delim_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/lc_delimiter.h"
#include "delim_kernel.hpp"
#include "packed_trip.hpp"

struct lc_delim {
    DelimConfig cfg;
};

extern "C" int lc_delim_create(const uint8_t* separator, uint32_t sep_len, uint8_t quote, int mode, uint32_t n_keys, lc_delim_t** out) {
    if (!out) return LC_ERR_ARG;
    *out = nullptr;
    DelimConfig c;
    if (!delimMakeConfig(separator, sep_len, quote, mode, n_keys, &c)) return LC_ERR_ARG;
    *out = new lc_delim{c};
    return LC_OK;
}
extern "C" void lc_delim_destroy(lc_delim_t* d) { delete d; }
extern "C" int lc_delim_uses_quote(const lc_delim_t* d) { return d ? d->cfg.useQuote : -1; }

static int launchSplit(const lc_delim* d, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status,
                       uint32_t* d_ncols, int32_t* d_spans, hipStream_t st) {
    const dim3 grid((n + lcdelim::kBlock - 1) / lcdelim::kBlock), block(lcdelim::kBlock);
    lcNoteKernel("delim_split_kernel");
    if (d->cfg.useQuote) hipLaunchKernelGGL(lcdelim::delim_split_kernel<true>, grid, block, 0, st, d->cfg, d_data, d_off, n, W, d_status, d_ncols, d_spans);
    else hipLaunchKernelGGL(lcdelim::delim_split_kernel<false>, grid, block, 0, st, d->cfg, d_data, d_off, n, W, d_status, d_ncols, d_spans);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

// ProcessorParseDelimiterNative.cpp:220-282 for n lines at once
extern "C" int lc_delim_split_device(lc_delim_t* d, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status,
                                     uint32_t* d_ncols, int32_t* d_spans, void* stream) {
    if (!d) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_status || !d_ncols || (W && !d_spans)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the delimiter parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchSplit(d, d_data, d_off, n, W, d_status, d_ncols, d_spans, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines
namespace {
thread_local PackedThread<struct DelimTag> tlsDelim;
}  // namespace

void lcDelimThreadRelease() { tlsDelim.release(); }

extern "C" int lc_delim_split_host(lc_delim_t* d, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status,
                                   uint32_t* ncols, int32_t* spans) {
    if (!d) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !ncols || (W && !spans)) return LC_ERR_ARG;
    auto& T = tlsDelim;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the delimiter parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t lineSpanBytes = size_t(W) * 8;
    // a chunk: 32 MiB of payload, 2^18 lines, 64 MiB of spans; down come the spans, the counts and the status bytes
    const PackedTripSpec spec{"lc_delim_split_host", "line", 1u << 18, 32u << 20, lineSpanBytes, 64u << 20, "hipMemcpyAsync(delimiter results)"};
    enum { kSpans, kNcols, kStatus };
    return packedTrip(
        T, spec, lines, len, n, {lineSpanBytes, 4, 1},
        [&](const PackedChunk& c) {
            return launchSplit(d, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, W, c.dResult<uint8_t>(kStatus),
                               c.dResult<uint32_t>(kNcols), c.dResult<int32_t>(kSpans), T.stream);
        },
        [&](PackedChunk& c) {
            if (W) std::memcpy(spans + size_t(c.next) * W * 2, c.hResult(kSpans, lineSpanBytes), size_t(c.cnt) * lineSpanBytes);
            std::memcpy(ncols + c.next, c.hResult(kNcols, 4), size_t(c.cnt) * 4);
            std::memcpy(status + c.next, c.hResult(kStatus, 1), c.cnt);
            return LC_OK;
        });
}
