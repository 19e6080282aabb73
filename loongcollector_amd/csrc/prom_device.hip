// prom_device.hip -- the engine level of the Prometheus text-line parser (include/lc_prom.h): the launch of prom_parse_kernel
// (prom_kernel.hpp) and the host entry's trip through a runner thread's pinned staging, with the host finish of the tokens the kernel
// left open.  Compiled like every other translation unit here: no fast-math (the one rounded operation of promNumberFinish must be an
// IEEE multiplication or division).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/lc_prom.h"
#include "packed_trip.hpp"
#include "prom_kernel.hpp"

static int launchParse(int honor, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, const lc_prom_out_t& o, hipStream_t st) {
    const dim3 grid((n + lcprom::kBlock - 1) / lcprom::kBlock), block(lcprom::kBlock);
    lcNoteKernel("prom_parse_kernel");
    const lcprom::PromOut out{o.status, o.flags, o.name, o.value, o.value_span, o.time_span, o.secs, o.nanos, o.nlabels, o.labels};
    hipLaunchKernelGGL(lcprom::prom_parse_kernel, grid, block, 0, st, d_data, d_off, n, W, honor ? 1 : 0, out);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}

static bool outComplete(const lc_prom_out_t* o, uint32_t W) {
    return o && o->status && o->flags && o->name && o->value && o->value_span && o->time_span && o->secs && o->nanos && o->nlabels && (!W || o->labels);
}
// aligned for the stores the kernel makes (a label: one 16-byte vector; a span: one 8-byte vector)
static bool outAligned(const lc_prom_out_t& o, uint32_t W) {
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    return !(misaligned(o.name, 8) || misaligned(o.value, 8) || misaligned(o.value_span, 8) || misaligned(o.time_span, 8) || misaligned(o.secs, 8) ||
             misaligned(o.nanos, 4) || misaligned(o.nlabels, 4) || (W && misaligned(o.labels, 16)));
}

extern "C" int lc_prom_parse_device(int honor_timestamps, const uint8_t* d_data, const int32_t* d_off, uint32_t n, const lc_prom_out_t* d_out, uint32_t W,
                                    void* stream) {
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !outComplete(d_out, W) || !outAligned(*d_out, W)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the Prometheus line parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    return launchParse(honor_timestamps, d_data, d_off, n, W, *d_out, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ host lines
namespace {
thread_local PackedThread<struct PromTag> tlsProm;
}  // namespace

void lcPromThreadRelease() { tlsProm.release(); }

extern "C" int lc_prom_parse_host(int honor_timestamps, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const lc_prom_out_t* out, uint32_t W,
                                  uint64_t* deferred_tokens) {
    if (deferred_tokens) *deferred_tokens = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !outComplete(out, W)) return LC_ERR_ARG;
    auto& T = tlsProm;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the Prometheus line parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t lineLabelBytes = size_t(W) * 16;
    // a chunk: 32 MiB of payload, 2^18 lines, 64 MiB of results
    const PackedTripSpec spec{"lc_prom_parse_host", "line", 1u << 18, 32u << 20, lineLabelBytes + 5 * 8 + 2 * 4 + 2, 64u << 20,
                              "hipMemcpyAsync(Prometheus line results)"};
    enum { kLabels, kName, kValue, kValueSpan, kTimeSpan, kSecs, kNanos, kNlabels, kStatus, kFlags };
    uint64_t deferred = 0;
    const int rc = packedTrip(
        T, spec, lines, len, n, {lineLabelBytes, 8, 8, 8, 8, 8, 4, 4, 1, 1},
        [&](const PackedChunk& c) {
            // (with W short of a line's labels the label block is only partly written: the copy down moves it whole, the caller reads
            // min(nlabels, W) entries of a line)
            const lc_prom_out_t d{c.dResult<uint8_t>(kStatus),    c.dResult<uint8_t>(kFlags),   c.dResult<int32_t>(kName),  c.dResult<uint64_t>(kValue),
                                  c.dResult<int32_t>(kValueSpan), c.dResult<int32_t>(kTimeSpan), c.dResult<int64_t>(kSecs), c.dResult<uint32_t>(kNanos),
                                  c.dResult<uint32_t>(kNlabels),  c.dResult<int32_t>(kLabels)};
            return launchParse(honor_timestamps, c.dIn, reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt), c.cnt, W, d, T.stream);
        },
        [&](PackedChunk& c) {
            const uint32_t* nl = reinterpret_cast<const uint32_t*>(c.hResult(kNlabels, 4));
            const uint8_t* hLabels = c.hResult(kLabels, lineLabelBytes);
            for (uint32_t i = 0; W && i < c.cnt; ++i) {  // only what the kernel wrote: the caller's array keeps what it held behind it
                const uint32_t k = nl[i] < W ? nl[i] : W;
                if (k) std::memcpy(out->labels + (size_t(c.next) + i) * W * 4, hLabels + size_t(i) * lineLabelBytes, size_t(k) * 16);
            }
            std::memcpy(out->name + size_t(c.next) * 2, c.hResult(kName, 8), size_t(c.cnt) * 8);
            std::memcpy(out->value + c.next, c.hResult(kValue, 8), size_t(c.cnt) * 8);
            std::memcpy(out->value_span + size_t(c.next) * 2, c.hResult(kValueSpan, 8), size_t(c.cnt) * 8);
            std::memcpy(out->time_span + size_t(c.next) * 2, c.hResult(kTimeSpan, 8), size_t(c.cnt) * 8);
            std::memcpy(out->secs + c.next, c.hResult(kSecs, 8), size_t(c.cnt) * 8);
            std::memcpy(out->nanos + c.next, c.hResult(kNanos, 4), size_t(c.cnt) * 4);
            std::memcpy(out->nlabels + c.next, nl, size_t(c.cnt) * 4);
            std::memcpy(out->status + c.next, c.hResult(kStatus, 1), c.cnt);
            std::memcpy(out->flags + c.next, c.hResult(kFlags, 1), c.cnt);
            // the host finish: exactly the tokens the kernel left open
            for (uint32_t i = 0; i < c.cnt; ++i) {
                const uint32_t li = c.next + i;
                if (!(out->flags[li] & (LC_PROM_VALUE_HOST | LC_PROM_TIME_HOST))) continue;
                PromLine r;
                promClear(r);
                r.status = out->status[li];
                r.flags = out->flags[li];
                r.value = out->value[li];
                r.secs = out->secs[li];
                r.nanos = out->nanos[li];
                r.valueSpan = PromSpan{out->value_span[size_t(li) * 2], out->value_span[size_t(li) * 2 + 1]};
                r.timeSpan = PromSpan{out->time_span[size_t(li) * 2], out->time_span[size_t(li) * 2 + 1]};
                deferred += promFinishHost(lines[li], r);
                out->status[li] = r.status;
                out->flags[li] = r.flags;
                out->value[li] = r.value;
                out->secs[li] = r.secs;
                out->nanos[li] = r.nanos;
            }
            return LC_OK;
        });
    if (deferred_tokens) *deferred_tokens = deferred;
    return rc;
}
