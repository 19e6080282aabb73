// trip_buffers.hpp -- a runner thread's device trips, written once for every owner (delim_device.hip, timestamp_device.hip,
// json_device.hip, apsara_device.hip, clog_device.hip, desens_device.hip, multiline_device.hip, processor_filter_gpu.cpp,
// processor_pipeline_gpu.cpp):
//   TripBuf       a grow-only pinned / device buffer
//   TripThread    the thread's stream, its device and its pinned completion word: begin() opens a host entry, end() closes a trip,
//                 release() gives everything back -- lc_thread_release() calls each owner's lc...ThreadRelease(), and so does the
//                 owner's destructor when the thread ends
//   tripCarve / tripInLayout / tripPackLines / tripLayout / tripCoalesce   the plan of the parsers' host entries: which lines a trip
//                 takes, their packed staging, where the result arrays lie, which shadow ranges come down in one copy -- pure
//                 arithmetic (tests/native/trip_plan_check.cpp); the loop that makes the trips is packed_trip.hpp
// HIP-light: the host translation units and the tests' host doubles include it as well.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/lc_regex_gpu.h"

// gpu_runtime.hip (what only the device translation units share: runtime_internal.hpp).  Nothing here sets the thread's error text: the
// device translation units word a failure with lcSetLastError / lcHipFail (lcTripBegin), the processors with their own strings.
void lcRegisterExitHook();                             // thread_local device resources: see gpu_runtime.hip
bool lcRuntimeUsable();                                // false once the process is exiting (the HIP runtime may be gone)
// The device a HOST entry point (processors, lc_*_match_host, multiline, filter, pipeline) runs on for the calling thread: the thread's
// binding (lc_runtime_bind_thread; first call binds by the process-wide policy), made current for the thread.  LC_OK or an error code.
int lcHostEntryDevice(int* dev);
// the ending of a zero-copy device trip (gpu_runtime.hip): a one-lane kernel behind everything on `stream` stores seq into the pinned word;
// the host spins on it (few waiters) or blocks in the runtime (many)
int lcQueueTripSignal(uint32_t* hFlag, uint32_t seq, hipStream_t stream);
int lcAwaitTripSignal(const uint32_t* hFlag, uint32_t seq, hipStream_t stream);
// the calling thread's next lc_regex_match_device_multi calls let the kernel read their (small) job tables from pinned memory
void lcSetJobTableInPlace(bool on);

struct TripBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t bytes) {
        if (p && cap >= bytes) return hipSuccess;
        release();
        const size_t want = bytes + (bytes >> 2) + 256;
        const hipError_t e = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

// The base of an owner's thread_local (struct XThread : TripThread<XThread>): the owner names its buffers in a release() of its own
// that hands them to releaseWith(), and calls that from its destructor (`if (live()) release();`) and from its lc...ThreadRelease().
struct TripBeginFail {  // why begin() did not return LC_OK, for the caller to word
    bool noDevice = false;          // lc_device_count() <= 0: the owner's "no CPU path" text
    hipError_t hip = hipSuccess;    // hipCall failed with this ...
    const char* hipCall = nullptr;  // ... (neither: the thread's binding failed, and lc_last_error() says why)
};

template <class Owner>
struct TripThread {
    hipStream_t stream = nullptr;
    int device = -1;
    TripBuf hFlag;  // the pinned completion word of an owner whose trips end with the signal (end())
    uint32_t seq = 0;
    const bool signalled;
    explicit TripThread(bool endsWithSignal) : signalled(endsWithSignal) { hFlag.pinned = true; }

    bool live() const { return lcRuntimeUsable() && stream; }  // (buffers are only ever allocated behind begin())

    // Opens a host entry: the thread's device into *dev; a thread that moved to another device starts over (its stream is destroyed, its
    // buffers -- allocated on the old device -- are released); the stream and the completion word on first use.  LC_OK, or the error
    // code with *why filled.
    int begin(int* dev, TripBeginFail* why) {
        if (lc_device_count() <= 0) {
            why->noDevice = true;
            return LC_ERR_NO_DEVICE;
        }
        const int rcDev = lcHostEntryDevice(dev);
        if (rcDev != LC_OK) return rcDev;
        if (stream && device != *dev) static_cast<Owner*>(this)->release();
        if (stream) return LC_OK;
        why->hipCall = "hipStreamCreateWithFlags(&T.stream, hipStreamNonBlocking)";
        why->hip = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (why->hip != hipSuccess) return LC_ERR_HIP;
        device = *dev;
        lcRegisterExitHook();
        if (signalled) {
            why->hipCall = "T.hFlag.ensure(64)";
            why->hip = hFlag.ensure(64);
            if (why->hip != hipSuccess) return LC_ERR_HIP;
            *static_cast<uint32_t*>(hFlag.p) = 0;
            seq = 0;
        }
        why->hipCall = nullptr;
        return LC_OK;
    }

    // A trip's end: the pinned word is stored by a one-lane kernel behind everything queued, and awaited.  rc: what queueing the trip gave;
    // on any failure the stream is drained, so that nothing queued here still touches the staging when the next call reuses it.
    int end(int rc) {
        uint32_t* word = static_cast<uint32_t*>(hFlag.p);
        const uint32_t s = ++seq;
        if (rc == LC_OK) rc = lcQueueTripSignal(word, s, stream);
        if (rc == LC_OK) rc = lcAwaitTripSignal(word, s, stream);
        if (rc != LC_OK) {
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
        }
        return rc;
    }

    void releaseWith(std::initializer_list<TripBuf*> bufs) {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
            stream = nullptr;
        }
        hFlag.release();
        for (TripBuf* b : bufs) b->release();
        device = -1;
    }
};

// ---- the plan of a packed-lines trip (packed_trip.hpp): the host entries lc_delim_split_host, lc_strptime_parse_host, lc_json_walk_host,
// lc_apsara_parse_host, lc_container_log_parse_host and lc_desens_apply_host
inline size_t tripRoundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Which lines line `from` and its successors (of n) add to a trip that holds *cnt lines of *bytes payload bytes already: the first always
// goes; then at most maxLines lines, maxBytes payload bytes and maxResultBytes of results at lineResultBytes each in the trip.
// false when that makes 2 GiB or more (the offsets are 32-bit).
inline bool tripCarve(const uint32_t* len, uint32_t from, uint32_t n, uint32_t maxLines, size_t maxBytes, size_t lineResultBytes,
                      size_t maxResultBytes, uint32_t* cnt, size_t* bytes) {
    const uint32_t had = *cnt;
    for (uint32_t at = from; at < n && *cnt < maxLines; ++at, ++*cnt) {
        if (*cnt != had && (*bytes + len[at] > maxBytes || (size_t(*cnt) + 1) * lineResultBytes > maxResultBytes)) break;
        *bytes += len[at];
    }
    return *bytes < (size_t(1) << 31);
}

// where the offsets lie behind `bytes` of payload: 64-byte aligned, at least 16 zero bytes behind the last line
inline size_t tripOffAt(size_t bytes) { return tripRoundUp(bytes + 16, 64); }

// Lines [first, first + cnt) back to back at hIn, their cnt offsets at hIn + offAt, zeroes between; returns the payload's byte count
// (the offset a line behind the last one would get).
inline size_t tripPackLines(uint8_t* hIn, size_t offAt, const uint8_t* const* lines, const uint32_t* len, uint32_t first, uint32_t cnt) {
    uint32_t* hOff = reinterpret_cast<uint32_t*>(hIn + offAt);
    size_t at = 0;
    for (uint32_t i = 0; i < cnt; ++i) {
        hOff[i] = uint32_t(at);
        if (len[first + i]) std::memcpy(hIn + at, lines[first + i], len[first + i]);
        at += len[first + i];
    }
    std::memset(hIn + at, 0, offAt - at);
    return at;
}
// (begin, end) = (0, len) of lines [first, first + cnt) at hIn + pairAt: the span pairs a kernel that takes spans reads
inline void tripPackPairs(uint8_t* hIn, size_t pairAt, const uint32_t* len, uint32_t first, uint32_t cnt) {
    int32_t* hPair = reinterpret_cast<int32_t*>(hIn + pairAt);
    for (uint32_t i = 0; i < cnt; ++i) {
        hPair[2 * i] = 0;
        hPair[2 * i + 1] = int32_t(len[first + i]);
    }
}

// The block that goes up: `payload` bytes, the offsets at offAt, and either their cnt + 1-th entry (pairAt == 0) or, 64-byte aligned
// behind cnt offsets, the lines' (begin, end) pairs.
struct TripInLayout {
    size_t offAt, pairAt, bytes;
};
inline TripInLayout tripInLayout(size_t payload, uint32_t cnt, bool pairs) {
    const size_t offAt = tripOffAt(payload);
    if (!pairs) return TripInLayout{offAt, 0, offAt + (size_t(cnt) + 1) * 4};
    const size_t pairAt = offAt + tripRoundUp(size_t(cnt) * 4, 64);
    return TripInLayout{offAt, pairAt, pairAt + size_t(cnt) * 8};
}

// The block that comes down: one array of cnt elements per entry of elemBytes, in that order, each 64-byte aligned.
struct TripLayout {
    static constexpr size_t kMaxArrays = 12;
    size_t at[kMaxArrays];
    size_t bytes;
};
inline TripLayout tripLayout(uint32_t cnt, const size_t* elemBytes, size_t arrays) {
    TripLayout L{};
    for (size_t k = 0; k < arrays && k < TripLayout::kMaxArrays; ++k) {
        L.at[k] = L.bytes;
        L.bytes += tripRoundUp(size_t(cnt) * elemBytes[k], 64);
    }
    return L;
}
inline TripLayout tripLayout(uint32_t cnt, std::initializer_list<size_t> elemBytes) { return tripLayout(cnt, elemBytes.begin(), elemBytes.size()); }

// The copies that bring the ascending ranges r[0..n) down: empty ranges (e <= b) are skipped, a range that begins within `gap` bytes
// of the copy before it extends that copy.  Returns the bytes the copies move.
struct TripRange {
    size_t b, e;
};
inline uint64_t tripCoalesce(const TripRange* r, size_t n, size_t gap, std::vector<TripRange>* copies) {
    copies->clear();
    for (size_t i = 0; i < n; ++i) {
        if (r[i].e <= r[i].b) continue;
        if (!copies->empty() && r[i].b <= copies->back().e + gap) copies->back().e = r[i].e;
        else copies->push_back(r[i]);
    }
    uint64_t moved = 0;
    for (const TripRange& c : *copies) moved += c.e - c.b;
    return moved;
}
