// packed_trip.hpp -- the trips of a host entry that takes host lines (lc_delim_split_host, lc_strptime_parse_host, lc_json_walk_host,
// lc_apsara_parse_host, lc_container_log_parse_host, lc_desens_apply_host), written once.  A chunk of the lines goes up packed in ONE
// copy (trip_buffers.hpp: tripCarve, tripInLayout, tripPackLines), the owner launches, the result arrays come down in ONE copy of one
// device block (tripLayout), the owner scatters them into the caller's arrays.  An owner brings its thread_local staging (PackedThread
// or a struct of its own over PackedShadowBuffers), a PackedTripSpec, a launch callback and a scatter callback; one whose result sizes
// are known only after its launches (desensitize) takes the input half alone: packedTripPlan, packedTripUpload, PackedChunk::advance.
// Device translation units only (lcHipFail, LC_HIP_TRY).
#pragma once

#include <string>
#include <vector>

#include "runtime_internal.hpp"
#include "trip_buffers.hpp"

// per runner thread: a stream, one pinned and one device block each way, the pinned completion word; grow-only
template <class Tag>
struct PackedThread : TripThread<PackedThread<Tag>> {
    TripBuf hIn, hOut, dIn, dOut;
    PackedThread() : TripThread<PackedThread<Tag>>(true) { hIn.pinned = hOut.pinned = true; }
    ~PackedThread() {
        if (this->live()) release();
    }
    void release() { this->releaseWith({&hIn, &hOut, &dIn, &dOut}); }
};
// ... and with a block each side for the bytes a kernel rewrites (the shadow).  The owner derives, and calls releaseBuffers() from a
// release() of its own (TripThread).
template <class Owner>
struct PackedShadowBuffers : TripThread<Owner> {
    TripBuf hIn, hOut, hShadow, dIn, dOut, dShadow;
    PackedShadowBuffers() : TripThread<Owner>(true) { hIn.pinned = hOut.pinned = hShadow.pinned = true; }
    void releaseBuffers() { this->releaseWith({&hIn, &hOut, &hShadow, &dIn, &dOut, &dShadow}); }
};

struct PackedTripSpec {
    const char* entry;       // the host entry's name and what it calls a line, for "<entry>: a <noun> of 2 GiB or more"
    const char* noun;
    uint32_t maxLines;       // a chunk's limits: tripCarve
    size_t maxBytes;
    size_t lineResultBytes;
    size_t maxResultBytes;
    const char* resultsCopy; // what a failed copy down is called in lc_last_error()
    bool leadIn = false;     // a chunk after the first starts one line early (its results are the owner's to drop: PackedChunk::lead)
    bool pairs = false;      // the lines' (begin, end) pairs go up behind the offsets, and no cnt + 1-th offset (tripInLayout)
};

struct PackedChunk {
    // the running state of the call
    uint32_t next = 0;       // the caller's first line that has no results yet
    size_t before = 0;       // the payload bytes of the lines before it: where its part of a caller's shadow begins
    uint64_t moved = 0;      // shadow bytes that came down so far (packedShadowDown)
    // the chunk: lines [first, first + cnt), of which the first `lead` had their results in the chunk before
    uint32_t lead = 0, first = 0, cnt = 0;
    size_t bytes = 0;        // payload
    TripInLayout in{};
    uint8_t* hIn = nullptr;
    uint8_t* dIn = nullptr;
    // its results (packedTrip)
    TripLayout out{};
    uint8_t* dOut = nullptr;
    const uint8_t* hOut = nullptr;

    const int32_t* hOff() const { return reinterpret_cast<const int32_t*>(hIn + in.offAt); }
    template <class V>
    V* dResult(size_t k) const { return reinterpret_cast<V*>(dOut + out.at[k]); }
    // the results of the chunk's first line that is not a lead-in, in array k of `each` bytes per line
    const uint8_t* hResult(size_t k, size_t each) const { return hOut + out.at[k] + size_t(lead) * each; }
    uint32_t got() const { return cnt - lead; }
    void advance(const uint32_t* len) {
        before += bytes - (lead ? len[first] : 0);
        next += got();
    }
};

// The input half, first step: which lines the chunk at c->next takes, and room for them in T.hIn / T.dIn.
template <class Thread>
int packedTripPlan(Thread& T, const PackedTripSpec& S, const uint32_t* len, uint32_t n, PackedChunk* c) {
    c->lead = S.leadIn && c->next ? 1u : 0u;
    c->first = c->next - c->lead;
    c->cnt = c->lead;
    c->bytes = c->lead ? len[c->first] : 0;
    if (!tripCarve(len, c->next, n, S.maxLines, S.maxBytes, S.lineResultBytes, S.maxResultBytes, &c->cnt, &c->bytes)) {
        lcSetLastError(std::string(S.entry) + ": a " + S.noun + " of 2 GiB or more");
        return LC_ERR_ARG;
    }
    c->in = tripInLayout(c->bytes, c->cnt, S.pairs);
    const size_t inBytes = c->in.bytes;
    LC_HIP_TRY(T.hIn.ensure(inBytes));
    LC_HIP_TRY(T.dIn.ensure(inBytes));
    c->hIn = static_cast<uint8_t*>(T.hIn.p);
    c->dIn = static_cast<uint8_t*>(T.dIn.p);
    return LC_OK;
}

// ... second step, once every block of the trip has its room: the lines packed, ONE copy up.
template <class Thread>
int packedTripUpload(Thread& T, const uint8_t* const* lines, const uint32_t* len, const PackedChunk& c) {
    uint8_t* hIn = c.hIn;
    uint8_t* dIn = c.dIn;
    const size_t inBytes = c.in.bytes;
    const size_t payload = tripPackLines(hIn, c.in.offAt, lines, len, c.first, c.cnt);
    if (c.in.pairAt) tripPackPairs(hIn, c.in.pairAt, len, c.first, c.cnt);
    else reinterpret_cast<uint32_t*>(hIn + c.in.offAt)[c.cnt] = uint32_t(payload);
    LC_HIP_TRY(hipMemcpyAsync(dIn, hIn, inBytes, hipMemcpyHostToDevice, T.stream));
    return LC_OK;
}

// A trip's end that brings the chunk's result block down: rc is what queueing the launches gave.
template <class Thread>
int packedTripDown(Thread& T, const PackedChunk& c, int rc, const char* what) {
    if (rc == LC_OK) {
        const hipError_t e = hipMemcpyAsync(T.hOut.p, c.dOut, c.out.bytes, hipMemcpyDeviceToHost, T.stream);
        if (e != hipSuccess) rc = lcHipFail(e, what);
    }
    return T.end(rc);
}

// Every chunk of lines[0..n): up, launch(c) -> rc, down, scatter(c) -> rc.  resultElemBytes: the result arrays' bytes per line, in
// the order c.out.at[] numbers them.  *moved: what packedShadowDown counted.
template <class Thread, class Launch, class Scatter>
int packedTrip(Thread& T, const PackedTripSpec& S, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
               std::initializer_list<size_t> resultElemBytes, Launch launch, Scatter scatter, uint64_t* moved = nullptr) {
    PackedChunk c;
    while (c.next < n) {
        if (const int rc = packedTripPlan(T, S, len, n, &c); rc != LC_OK) return rc;
        c.out = tripLayout(c.cnt, resultElemBytes);
        const size_t outBytes = c.out.bytes;
        LC_HIP_TRY(T.hOut.ensure(outBytes));
        LC_HIP_TRY(T.dOut.ensure(outBytes));
        c.dOut = static_cast<uint8_t*>(T.dOut.p);
        c.hOut = static_cast<const uint8_t*>(T.hOut.p);
        if (const int rc = packedTripUpload(T, lines, len, c); rc != LC_OK) return rc;
        int rc = packedTripDown(T, c, launch(c), S.resultsCopy);
        if (rc == LC_OK) rc = scatter(c);
        if (rc != LC_OK) return rc;
        c.advance(len);
    }
    if (moved) *moved = c.moved;
    return LC_OK;
}

// The rewritten bytes of a chunk: only the ranges (ascending, relative to the chunk's payload) come down from T.dShadow, neighbours
// within kShadowGap in one copy -- a trip of its own -- and land in the caller's shadow behind c->before.
constexpr uint32_t kShadowGap = 4096;
template <class Thread>
int packedShadowDown(Thread& T, PackedChunk* c, const std::vector<TripRange>& spans, uint8_t* shadow, const char* what) {
    if (spans.empty()) return LC_OK;
    std::vector<TripRange> copies;
    const uint64_t moving = tripCoalesce(spans.data(), spans.size(), kShadowGap, &copies);
    const size_t offAt = c->in.offAt;
    LC_HIP_TRY(T.hShadow.ensure(offAt));
    uint8_t* hShadow = static_cast<uint8_t*>(T.hShadow.p);
    const uint8_t* dShadow = static_cast<const uint8_t*>(T.dShadow.p);
    int rc = LC_OK;
    for (const TripRange& r : copies) {
        const hipError_t e = hipMemcpyAsync(hShadow + r.b, dShadow + r.b, r.e - r.b, hipMemcpyDeviceToHost, T.stream);
        if (e != hipSuccess) {
            rc = lcHipFail(e, what);
            break;
        }
    }
    if (!copies.empty()) {
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
    }
    c->moved += moving;
    for (const TripRange& r : spans)
        if (r.e > r.b) std::memcpy(shadow + c->before + r.b, hShadow + r.b, r.e - r.b);
    return LC_OK;
}
