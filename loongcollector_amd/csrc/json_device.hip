// json_device.hip -- the engine level of the JSON parser (include/lc_json.h): the launches of json_walk_kernel (json_kernel.hpp) and
// the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lc_json.h"
#include "json_kernel.hpp"
#include "packed_trip.hpp"

namespace {
// the second launch's nesting stacks: one block of kDeepScratchBytes (2 MiB) per (device, stream) that has queued a walk, allocated
// at its first walk.  Per stream, because launches of two streams may run at once and a lane's slice belongs to one launch at a time;
// launches of one stream run in order.  A runner thread's block goes when the thread's stream goes; a caller's stream keeps its block
// for the life of the process.
struct DeepScratch {
    int device;
    hipStream_t stream;
    uint32_t* p;
};
std::mutex gDeepMutex;
std::vector<DeepScratch> gDeep;

int deepScratchFor(int dev, hipStream_t st, uint32_t** out) {
    std::lock_guard<std::mutex> lock(gDeepMutex);
    for (const DeepScratch& d : gDeep)
        if (d.device == dev && d.stream == st) {
            *out = d.p;
            return LC_OK;
        }
    void* p = nullptr;
    LC_HIP_TRY(hipMalloc(&p, lcjsonk::kDeepScratchBytes));
    gDeep.push_back(DeepScratch{dev, st, static_cast<uint32_t*>(p)});
    *out = static_cast<uint32_t*>(p);
    return LC_OK;
}
void deepScratchForget(int dev, hipStream_t st) {  // a stream that is about to be destroyed
    std::lock_guard<std::mutex> lock(gDeepMutex);
    for (size_t i = 0; i < gDeep.size(); ++i)
        if (gDeep[i].device == dev && gDeep[i].stream == st) {
            (void)hipFree(gDeep[i].p);
            gDeep.erase(gDeep.begin() + i);
            return;
        }
}

int launchWalk(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_nmembers,
               uint32_t* d_errpos, lc_json_member_t* d_records, uint8_t* d_shadow, hipStream_t st) {
    const dim3 grid((n + lcjsonk::kBlock - 1) / lcjsonk::kBlock), block(lcjsonk::kBlock);
    lcNoteKernel("json_walk_kernel");
    hipLaunchKernelGGL(lcjsonk::json_walk_kernel<false>, grid, block, 0, st, d_data, d_off, n, W, d_status, d_nmembers, d_errpos, d_records,
                       d_shadow, static_cast<uint32_t*>(nullptr));
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}
int launchDeep(int dev, const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_nmembers,
               uint32_t* d_errpos, lc_json_member_t* d_records, uint8_t* d_shadow, hipStream_t st) {
    uint32_t* scratch = nullptr;
    const int rc = deepScratchFor(dev, st, &scratch);
    if (rc != LC_OK) return rc;
    const uint32_t blocks = (n + lcjsonk::kBlock - 1) / lcjsonk::kBlock;
    const dim3 grid(blocks < lcjsonk::kDeepBlocks ? blocks : lcjsonk::kDeepBlocks), block(lcjsonk::kBlock);
    lcNoteKernel("json_walk_kernel");
    hipLaunchKernelGGL(lcjsonk::json_walk_kernel<true>, grid, block, 0, st, d_data, d_off, n, W, d_status, d_nmembers, d_errpos, d_records,
                       d_shadow, scratch);
    LC_HIP_TRY(hipGetLastError());
    return LC_OK;
}
}  // namespace

// ProcessorParseJsonNative.cpp:257-366 for n lines at once
extern "C" int lc_json_walk_device(const uint8_t* d_data, const int32_t* d_off, uint32_t n, uint32_t W, uint8_t* d_status, uint32_t* d_nmembers,
                                   uint32_t* d_errpos, lc_json_member_t* d_records, uint8_t* d_shadow, void* stream) {
    if (n == 0) return LC_OK;
    if (!d_data || !d_off || !d_status || !d_nmembers || !d_errpos || !d_shadow || (W && !d_records)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the JSON parser has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);  // (never switches devices; refuses a pointer of another one)
    if (rcDev != LC_OK) return rcDev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = launchWalk(d_data, d_off, n, W, d_status, d_nmembers, d_errpos, d_records, d_shadow, st);
    if (rc != LC_OK) return rc;
    return launchDeep(dev, d_data, d_off, n, W, d_status, d_nmembers, d_errpos, d_records, d_shadow, st);
}

// ------------------------------------------------------------------------------------------------ host lines
namespace {
struct JsonThread : PackedShadowBuffers<JsonThread> {
    ~JsonThread() {
        if (live()) release();
    }
    void release() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            deepScratchForget(device, stream);  // (before the stream is destroyed: the block is found by it)
        }
        releaseBuffers();
    }
};
thread_local JsonThread tlsJson;
}  // namespace

void lcJsonThreadRelease() { tlsJson.release(); }

extern "C" int lc_json_walk_host(const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* nmembers,
                                 uint32_t* errpos, lc_json_member_t* records, uint8_t* shadow, uint64_t* shadow_bytes_moved) {
    if (shadow_bytes_moved) *shadow_bytes_moved = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !nmembers || !errpos || !shadow || (W && !records)) return LC_ERR_ARG;
    JsonThread& T = tlsJson;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the JSON parser has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    const size_t lineRecordBytes = size_t(W) * sizeof(lc_json_member_t);
    // a chunk: 32 MiB of payload, 2^18 lines, 64 MiB of records; down come records, counts, error offsets and status bytes
    const PackedTripSpec spec{"lc_json_walk_host", "line", 1u << 18, 32u << 20, lineRecordBytes, 64u << 20, "hipMemcpyAsync(JSON results)"};
    enum { kRecords, kCount, kErr, kStatus };
    const auto launch = [&](const PackedChunk& c, bool deep) {
        const int32_t* dOff = reinterpret_cast<const int32_t*>(c.dIn + c.in.offAt);
        uint8_t* dShadow = static_cast<uint8_t*>(T.dShadow.p);
        uint8_t* dStatus = c.dResult<uint8_t>(kStatus);
        uint32_t* dCount = c.dResult<uint32_t>(kCount);
        uint32_t* dErr = c.dResult<uint32_t>(kErr);
        lc_json_member_t* dRec = c.dResult<lc_json_member_t>(kRecords);
        if (deep) return launchDeep(dev, c.dIn, dOff, c.cnt, W, dStatus, dCount, dErr, dRec, dShadow, T.stream);
        return launchWalk(c.dIn, dOff, c.cnt, W, dStatus, dCount, dErr, dRec, dShadow, T.stream);
    };
    return packedTrip(
        T, spec, lines, len, n, {lineRecordBytes, 4, 4, 1},
        [&](const PackedChunk& c) {
            const size_t offAt = c.in.offAt;
            LC_HIP_TRY(T.dShadow.ensure(offAt));
            return launch(c, false);
        },
        [&](PackedChunk& c) {
            // lines nested deeper than the first launch's registers reach: the second launch, over the chunk that still lies on the device
            if (std::memchr(c.hResult(kStatus, 1), LC_JSON_DEEP, c.cnt)) {
                const int rc = packedTripDown(T, c, launch(c, true), "hipMemcpyAsync(JSON results, second launch)");
                if (rc != LC_OK) return rc;
            }
            if (W) std::memcpy(records + size_t(c.next) * W, c.hResult(kRecords, lineRecordBytes), size_t(c.cnt) * lineRecordBytes);
            std::memcpy(nmembers + c.next, c.hResult(kCount, 4), size_t(c.cnt) * 4);
            std::memcpy(errpos + c.next, c.hResult(kErr, 4), size_t(c.cnt) * 4);
            std::memcpy(status + c.next, c.hResult(kStatus, 1), c.cnt);
            // the unescaped bytes: only the escaped spans' come down (in ascending order: members come in document order)
            std::vector<TripRange> spans;
            for (uint32_t i = 0; i < c.cnt; ++i) {
                if (status[c.next + i] != LC_JSON_OK) continue;
                const uint32_t m = nmembers[c.next + i] < W ? nmembers[c.next + i] : W;
                const lc_json_member_t* row = records + size_t(c.next + i) * W;
                const size_t at = size_t(c.hOff()[i]);
                for (uint32_t k = 0; k < m; ++k) {
                    if (row[k].key_begin & LC_JSON_ESCAPED) spans.push_back(TripRange{at + (row[k].key_begin & ~LC_JSON_ESCAPED), at + row[k].key_end});
                    if (row[k].type == LC_JSON_STRING && (row[k].val_begin & LC_JSON_ESCAPED))
                        spans.push_back(TripRange{at + (row[k].val_begin & ~LC_JSON_ESCAPED), at + row[k].val_end});
                }
            }
            return packedShadowDown(T, &c, spans, shadow, "hipMemcpyAsync(JSON unescaped bytes)");
        },
        shadow_bytes_moved);
}
