// json_device.hip -- the engine level of the JSON parser (include/lc_json.h): the launches of json_walk_kernel (json_kernel.hpp) and
// the host entry's trip through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lc_json.h"
#include "json_kernel.hpp"
#include "runtime_internal.hpp"
#include "trip_buffers.hpp"

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
// per runner thread: a stream, pinned and device blocks each way, the pinned completion word; grow-only
struct JsonThread : TripThread<JsonThread> {
    TripBuf hIn, hOut, hShadow, dIn, dOut, dShadow;
    JsonThread() : TripThread(true) { hIn.pinned = hOut.pinned = hShadow.pinned = true; }
    ~JsonThread() {
        if (live()) release();
    }
    void release() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            deepScratchForget(device, stream);  // (before the stream is destroyed: the block is found by it)
        }
        releaseWith({&hIn, &hOut, &hShadow, &dIn, &dOut, &dShadow});
    }
};
thread_local JsonThread tlsJson;

constexpr size_t kChunkBytes = 32u << 20;    // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;   // and at most this many lines
constexpr size_t kChunkRecordBytes = 64u << 20;
constexpr uint32_t kShadowGap = 4096;        // two escaped spans closer than this come down in one copy
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
    uint32_t next = 0;
    size_t shadowAt = 0;  // where line `next`'s part of the caller's shadow begins
    uint64_t moved = 0;
    while (next < n) {
        // a chunk: the lines back to back, then (64-byte aligned) their n + 1 offsets -- ONE copy up; records, counts, error offsets and
        // status bytes in one device block -- ONE copy down
        uint32_t cnt = 0;
        size_t bytes = 0;
        if (!tripCarve(len, next, n, kChunkLines, kChunkBytes, lineRecordBytes, kChunkRecordBytes, &cnt, &bytes)) {
            lcSetLastError("lc_json_walk_host: a line of 2 GiB or more");
            return LC_ERR_ARG;
        }
        const size_t offAt = tripOffAt(bytes);
        const size_t inBytes = offAt + (size_t(cnt) + 1) * 4;
        const size_t countAt = tripRoundUp(size_t(cnt) * lineRecordBytes, 64);
        const size_t errAt = countAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t statusAt = errAt + tripRoundUp(size_t(cnt) * 4, 64);
        const size_t outBytes = statusAt + tripRoundUp(cnt, 64);
        LC_HIP_TRY(T.hIn.ensure(inBytes));
        LC_HIP_TRY(T.dIn.ensure(inBytes));
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        LC_HIP_TRY(T.dShadow.ensure(offAt));
        uint8_t* hIn = static_cast<uint8_t*>(T.hIn.p);
        int32_t* hOff = reinterpret_cast<int32_t*>(hIn + offAt);
        hOff[cnt] = int32_t(tripPackLines(hIn, offAt, lines, len, next, cnt));
        uint8_t* dIn = static_cast<uint8_t*>(T.dIn.p);
        uint8_t* dOut = static_cast<uint8_t*>(T.dOut.p);
        uint8_t* dShadow = static_cast<uint8_t*>(T.dShadow.p);
        const int32_t* dOff = reinterpret_cast<const int32_t*>(dIn + offAt);
        uint8_t* dStatus = dOut + statusAt;
        uint32_t* dCount = reinterpret_cast<uint32_t*>(dOut + countAt);
        uint32_t* dErr = reinterpret_cast<uint32_t*>(dOut + errAt);
        lc_json_member_t* dRec = reinterpret_cast<lc_json_member_t*>(dOut);
        LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
        int rc = launchWalk(dIn, dOff, cnt, W, dStatus, dCount, dErr, dRec, dShadow, T.stream);
        if (rc == LC_OK) {
            const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(JSON results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint8_t* hOut = static_cast<const uint8_t*>(T.hOut.p);
        // lines nested deeper than the first launch's registers reach: the second launch, over the chunk that still lies on the device
        if (std::memchr(hOut + statusAt, LC_JSON_DEEP, cnt)) {
            rc = launchDeep(dev, dIn, dOff, cnt, W, dStatus, dCount, dErr, dRec, dShadow, T.stream);
            if (rc == LC_OK) {
                const hipError_t e = hipMemcpyAsync(T.hOut.p, dOut, outBytes, hipMemcpyDeviceToHost, T.stream);
                if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(JSON results, second launch)");
            }
            rc = T.end(rc);
            if (rc != LC_OK) return rc;
        }
        if (W) std::memcpy(records + size_t(next) * W, hOut, size_t(cnt) * lineRecordBytes);
        std::memcpy(nmembers + next, hOut + countAt, size_t(cnt) * 4);
        std::memcpy(errpos + next, hOut + errAt, size_t(cnt) * 4);
        std::memcpy(status + next, hOut + statusAt, cnt);
        // the unescaped bytes: only the escaped spans' come down, neighbours within kShadowGap in one copy
        struct Range {
            size_t b, e;
        };
        std::vector<Range> spans, copies;
        for (uint32_t i = 0; i < cnt; ++i) {
            if (status[next + i] != LC_JSON_OK) continue;
            const uint32_t m = nmembers[next + i] < W ? nmembers[next + i] : W;
            const lc_json_member_t* row = records + size_t(next + i) * W;
            for (uint32_t k = 0; k < m; ++k) {
                if (row[k].key_begin & LC_JSON_ESCAPED)
                    spans.push_back(Range{size_t(hOff[i]) + (row[k].key_begin & ~LC_JSON_ESCAPED), size_t(hOff[i]) + row[k].key_end});
                if (row[k].type == LC_JSON_STRING && (row[k].val_begin & LC_JSON_ESCAPED))
                    spans.push_back(Range{size_t(hOff[i]) + (row[k].val_begin & ~LC_JSON_ESCAPED), size_t(hOff[i]) + row[k].val_end});
            }
        }
        if (!spans.empty()) {
            for (const Range& r : spans) {  // (in ascending order: members come in document order)
                if (r.e <= r.b) continue;
                if (!copies.empty() && r.b <= copies.back().e + kShadowGap) copies.back().e = r.e;
                else copies.push_back(r);
            }
            LC_HIP_TRY(T.hShadow.ensure(offAt));
            uint8_t* hShadow = static_cast<uint8_t*>(T.hShadow.p);
            rc = LC_OK;
            for (const Range& c : copies) {
                const hipError_t e = hipMemcpyAsync(hShadow + c.b, dShadow + c.b, c.e - c.b, hipMemcpyDeviceToHost, T.stream);
                if (e != hipSuccess) {
                    rc = lcHipFail(e, "hipMemcpyAsync(JSON unescaped bytes)");
                    break;
                }
                moved += c.e - c.b;
            }
            if (!copies.empty()) {
                rc = T.end(rc);
                if (rc != LC_OK) return rc;
            }
            for (const Range& r : spans)
                if (r.e > r.b) std::memcpy(shadow + shadowAt + r.b, hShadow + r.b, r.e - r.b);
        }
        shadowAt += bytes;
        next += cnt;
    }
    if (shadow_bytes_moved) *shadow_bytes_moved = moved;
    return LC_OK;
}
