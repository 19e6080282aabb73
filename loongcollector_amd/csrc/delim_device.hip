// delim_device.hip -- the engine level of the delimiter parser (include/lc_delimiter.h): the handle, the launch of
// delim_split_kernel (delim_kernel.hpp) and the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/lc_delimiter.h"
#include "delim_kernel.hpp"
#include "runtime_internal.hpp"
#include "trip_buffers.hpp"

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
// per runner thread: a stream, one pinned and one device block each way, the pinned completion word; grow-only
struct DelimThread : TripThread<DelimThread> {
    TripBuf hIn, hOut, dIn, dOut;
    DelimThread() : TripThread(true) { hIn.pinned = hOut.pinned = true; }
    ~DelimThread() {
        if (live()) release();
    }
    void release() { releaseWith({&hIn, &hOut, &dIn, &dOut}); }
};
thread_local DelimThread tlsDelim;

constexpr size_t kChunkBytes = 32u << 20;    // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;   // and at most this many lines
constexpr size_t kChunkSpanBytes = 64u << 20;
}  // namespace

void lcDelimThreadRelease() { tlsDelim.release(); }

extern "C" int lc_delim_split_host(lc_delim_t* d, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status,
                                   uint32_t* ncols, int32_t* spans) {
    if (!d) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !ncols || (W && !spans)) return LC_ERR_ARG;
    DelimThread& T = tlsDelim;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the delimiter parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t lineSpanBytes = size_t(W) * 8;
    uint32_t next = 0;
    while (next < n) {
        // a chunk: the lines back to back, then (64-byte aligned) their n + 1 offsets -- ONE copy up; spans, counts and status bytes
        // in one device block -- ONE copy down
        uint32_t cnt = 0;
        size_t bytes = 0;
        if (!tripCarve(len, next, n, kChunkLines, kChunkBytes, lineSpanBytes, kChunkSpanBytes, &cnt, &bytes)) {
            lcSetLastError("lc_delim_split_host: a line of 2 GiB or more");
            return LC_ERR_ARG;
        }
        const size_t offAt = tripOffAt(bytes);
        const size_t inBytes = offAt + (size_t(cnt) + 1) * 4;
        const size_t ncolsAt = tripRoundUp(size_t(cnt) * lineSpanBytes, 64);
        const size_t statusAt = ncolsAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t outBytes = statusAt + tripRoundUp(cnt, 64);
        LC_HIP_TRY(T.hIn.ensure(inBytes));
        LC_HIP_TRY(T.dIn.ensure(inBytes));
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
        reinterpret_cast<int32_t*>(hIn + offAt)[cnt] = int32_t(tripPackLines(hIn, offAt, lines, len, next, cnt));
        uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
        uint8_t* dOut = static_cast<uint8_t*>(T.dOut.p);
        LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
        int rc = launchSplit(d, dIn, reinterpret_cast<const int32_t*>(dIn + offAt), cnt, W, dOut + statusAt,
                             reinterpret_cast<uint32_t*>(dOut + ncolsAt), reinterpret_cast<int32_t*>(dOut), T.stream);
        if (rc == LC_OK) {
            const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(delimiter results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint8_t* hOut = static_cast<const uint8_t*>(T.hOut.p);
        if (W) std::memcpy(spans + size_t(next) * W * 2, hOut, size_t(cnt) * lineSpanBytes);
        std::memcpy(ncols + next, hOut + ncolsAt, size_t(cnt) * 4);
        std::memcpy(status + next, hOut + statusAt, cnt);
        next += cnt;
    }
    return LC_OK;
}
