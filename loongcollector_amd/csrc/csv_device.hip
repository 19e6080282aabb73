// csv_device.hip -- the engine level of the CSV decoder (include/csv/lc_csv.h): the launch of csv_split_kernel (csv_kernel.hpp) and the
// host entry's trip through a runner thread's pinned staging.  The handle and everything the Go plugin does around the read live in
// processor_csv_gpu.cpp.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/csv/lc_csv.h"
#include "csv_kernel.hpp"
#include "packed_trip.hpp"
#include "processor_csv_gpu.hpp"

static int launchSplit(const CsvConfig& cfg, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_count,
                       int32_t* d_fields, hipStream_t st) {
    const dim3 grid((n + lccsv::kBlock - 1) / lccsv::kBlock), block(lccsv::kBlock);
    lcNoteKernel("csv_split_kernel");
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, cfg.sepWord, cfg.sepLen, d_data, d_off, n, W, d_status, d_count, d_fields);
    };
    if (cfg.trim) launch(lccsv::csv_split_kernel<true>);
    else launch(lccsv::csv_split_kernel<false>);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

static int refuseInvalidDelimiter(const lc_csv_t* p) {
    if (!lcCsvConfig(p).invalidDelim) return LC_OK;
    lcSetLastError("csv: invalid field or comment delimiter");
    return LC_ERR_UNSUPPORTED;
}

// r.Read() (encoding/csv) for n values at once
extern "C" int lc_csv_device(const lc_csv_t* p, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_count,
                             int32_t* d_fields, void* stream) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_status || !d_count || (W && !d_fields)) return LC_ERR_ARG;
    // aligned for the stores the kernel makes (a row: one 8-byte vector)
    if ((reinterpret_cast<uintptr_t>(d_count) & 3u) || (W && (reinterpret_cast<uintptr_t>(d_fields) & 7u))) return LC_ERR_ARG;
    const int rcDelim = refuseInvalidDelimiter(p);
    if (rcDelim != LC_OK) return rcDelim;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the CSV decoder has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchSplit(lcCsvConfig(p), d_data, d_off, n, W, d_status, d_count, d_fields, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
thread_local PackedThread<struct CsvTag> tlsCsv;
}  // namespace

extern "C" void lc_csv_thread_release(void) { tlsCsv.release(); }

extern "C" int lc_csv_host(const lc_csv_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* count,
                           int32_t* fields) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !count || (W && !fields)) return LC_ERR_ARG;
    const int rcDelim = refuseInvalidDelimiter(p);
    if (rcDelim != LC_OK) return rcDelim;
    auto& T = tlsCsv;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the CSV decoder has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t valueRowBytes = size_t(W) * 8;
    // a chunk: 32 MiB of payload, 2^18 values, 64 MiB of rows; down come the rows, the counts and the status bytes
    const PackedTripSpec spec{"lc_csv_host", "value", 1u << 18, 32u << 20, valueRowBytes + 4 + 1, 64u << 20, "hipMemcpyAsync(CSV results)"};
    enum { kRows, kCount, kStatus };
    const CsvConfig& cfg = lcCsvConfig(p);
    return packedTrip(
        T, spec, lines, len, n, {valueRowBytes, 4, 1},
        [&](const PackedChunk& c) {
            return launchSplit(cfg, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, W, c.dResult<uint8_t>(kStatus),
                               c.dResult<uint32_t>(kCount), c.dResult<int32_t>(kRows), T.stream);
        },
        [&](PackedChunk& c) {
            const uint32_t* np = reinterpret_cast<const uint32_t*>(c.hResult(kCount, 4));
            const uint8_t* st = c.hResult(kStatus, 1);
            const uint8_t* hRows = c.hResult(kRows, valueRowBytes);
            for (uint32_t i = 0; W && i < c.cnt; ++i) {  // only what the kernel wrote: the caller's array keeps what it held behind it
                if (st[i] != LC_CSV_OK) continue;        // (count and rows of an error value are unspecified)
                const uint32_t k = np[i] < W ? np[i] : W;
                if (k) std::memcpy(fields + (size_t(c.next) + i) * W * 2, hRows + size_t(i) * valueRowBytes, size_t(k) * 8);
            }
            std::memcpy(count + c.next, np, size_t(c.cnt) * 4);
            std::memcpy(status + c.next, st, c.cnt);
            return LC_OK;
        });
}
