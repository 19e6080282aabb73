// grok_device.hip -- device half of the Grok processor (include/lc_grok.h):
// ProcessorGrok.processGrok (plugins/processor/grok/processor_grok.go:148-194) for a whole batch of values.
//
// Two ways through a Match list, same results:
//   * speculative (default, lists of up to 64 entries): grok_plan_kernel.hpp -- one literal pass, ONE launch for the screens of
//     all entries, then every surviving (entry, value) pair evaluated at the same time on a few streams, the first contributing
//     entry per value taken at the end.  Round control stays on the device; the host synchronises twice per batch.
//   * sequential: grok_kernel.hpp -- the list walked entry by entry over the values still undecided (a host round trip per
//     filter, screen and search round).
// The regex kernels themselves (tdfa_* / nfa_*) live in gpu_runtime.hip and are reached through lcMatchOnStream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "grok_kernel.hpp"
#include "grok_plan_host.hpp"
#include "grok_plan_kernel.hpp"
#include "grok_runtime.hpp"
#include "group_combiner.hpp"
#include "regex_handle.hpp"
#include "runtime_internal.hpp"
#include "tdfa_l2_layout.h"

#define HIP_TRY LC_HIP_TRY

namespace {
size_t alignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

thread_local GrokBatchStats tlsStats;
// lcGrokMatchHost asks the device call to queue the copies of its results (pinned host memory) behind its last kernels, so that the
// call's final synchronisation covers them
struct GrokTailCopy {
    int32_t* hPattern = nullptr;
    int32_t* hFirst = nullptr;
    bool armed = false, done = false;
    uint32_t nextra = 0;
};
thread_local GrokTailCopy tlsTail;
hipError_t syncCounted(hipStream_t st) {
    ++tlsStats.hostSyncs;
    return hipStreamSynchronize(st);
}
}  // namespace

GrokBatchStats lcGrokLastBatchStats() { return tlsStats; }

// Scratch layout.  Sequential path: caps int32[n][row] | status u8[n] (padded) | from, nmatch, tried, next, roundA, roundB,
// unanchored : u32[n] each | counters u32[64] | perPattern u32[64] | masks u64[n] | work u32[1024].  The speculative path only uses the tail
// (counters .. masks) plus winner / undecided u32[n] carved from the head; its per-entry arrays come from the thread's arena.
size_t lcGrokScratchBytes(uint32_t n, uint32_t rowInts) {
    const size_t m = n ? n : 1;
    return alignUp(m * rowInts * 4, 256) + alignUp(m, 256) + 7 * alignUp(m * 4, 256) + 512 + alignUp(m * 8, 256) + 4096;
}

// ------------------------------------------------------------------------------------------------ per-handle device state
struct GrokDeviceState {
    std::mutex m;
    bool literalsBuilt = false;
    std::vector<uint32_t> literalBlob;           // empty: the list is not indexable
    void* dLiteral[kLcMaxDevices] = {};
    // screens of the speculative path: per device, a table of GrokScreenDev (at most one screen per entry)
    bool screensBuilt[kLcMaxDevices] = {};
    void* dScreens[kLcMaxDevices] = {};
    uint32_t nScreens[kLcMaxDevices] = {};
    uint32_t screenLdsBytes[kLcMaxDevices] = {};  // largest staged table
    std::vector<GrokScreenDev> hostScreens[kLcMaxDevices];  // the same table on the host (kernel arguments of the remainder screens)
    // lcGrokMatchHost: the groups of concurrent runner threads travel as ONE batch per device (group_combiner.hpp): a worker thread
    // per (processor, device) owns the plan, the streams and the pinned staging
    struct HostJob;
    struct HostCombiner;
    HostCombiner* combiner[kLcMaxDevices] = {};
};

static void grokFreeCombiners(GrokDeviceState* s);
GrokDeviceState* lcGrokStateCreate() { return new GrokDeviceState(); }
void lcGrokStateFree(GrokDeviceState* s) {
    if (!s) return;
    grokFreeCombiners(s);  // (the worker threads end first: they use the tables freed below)
    if (lcRuntimeUsable()) {
        int cur = 0;
        const bool haveCur = hipGetDevice(&cur) == hipSuccess;
        for (int d = 0; d < kLcMaxDevices; ++d) {
            if (!s->dLiteral[d] && !s->dScreens[d]) continue;
            if (hipSetDevice(d) != hipSuccess) continue;
            if (s->dLiteral[d]) (void)hipFree(s->dLiteral[d]);
            if (s->dScreens[d]) (void)hipFree(s->dScreens[d]);
        }
        if (haveCur) (void)hipSetDevice(cur);
    }
    delete s;
}

namespace {
// device blob of the list's literal index, or nullptr (more than 64 entries, no literal at all, automaton too large).  Built once
// per handle, uploaded once per device; freed with the handle.
int grokLiteralIndex(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, int dev, const uint32_t** out) {
    *out = nullptr;
    static const bool off = getenv("LC_GROK_NO_LITERAL_INDEX") != nullptr;
    if (off || patterns.size() > 64) return LC_OK;
    std::lock_guard<std::mutex> g(state->m);
    if (!state->literalsBuilt) {
        std::vector<std::string> lits;
        size_t withLiteral = 0;
        for (const auto& gp : patterns) {
            lits.push_back(lcGrokLiteralOf(gp.re));
            withLiteral += !lits.back().empty();
        }
        if (withLiteral >= 2) state->literalBlob = lcBuildGrokLiteralBlob(lits);
        state->literalsBuilt = true;
    }
    if (state->literalBlob.empty()) return LC_OK;
    if (!state->dLiteral[dev]) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, state->literalBlob.size() * 4));
        const hipError_t e = hipMemcpy(p, state->literalBlob.data(), state->literalBlob.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return lcHipFail(e, "hipMemcpy(literal index)");
        }
        state->dLiteral[dev] = p;
    }
    *out = static_cast<const uint32_t*>(state->dLiteral[dev]);
    return LC_OK;
}
}  // namespace

// ---- the sequential path: the Match list walked entry by entry over the values still undecided (the control flow of
// grok_kernel.hpp).  Lists of more than 64 entries, and handles configured with "Speculative": false.
static int grokMatchSequential(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, const GrokOptions& opts,
                               uint32_t row, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n,
                               int32_t* d_pattern, int32_t* d_first, int32_t* d_extra, uint32_t extraCap, uint32_t* d_nextra,
                               void* d_scratch, hipStream_t st, int dev) {

    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    int32_t* caps = reinterpret_cast<int32_t*>(base);
    base += alignUp(size_t(n) * row * 4, 256);
    uint8_t* status = base;
    base += alignUp(n, 256);
    uint32_t* lists[7];
    for (auto& l : lists) {
        l = reinterpret_cast<uint32_t*>(base);
        base += alignUp(size_t(n) * 4, 256);
    }
    uint32_t *from = lists[0], *nmatch = lists[1], *tried = lists[2], *next = lists[3], *roundIn = lists[4],
             *roundOut = lists[5], *unanchored = lists[6];
    uint32_t* counters = reinterpret_cast<uint32_t*>(base);
    base += 256;
    uint32_t* perPattern = reinterpret_cast<uint32_t*>(base);  // [64]: values that carry each entry's literal (literal index pass)
    base += 256;
    uint64_t* masks = reinterpret_cast<uint64_t*>(base);

    const uint32_t gridAll = (n + kGrokBlock - 1) / kGrokBlock;
    hipLaunchKernelGGL(grok_init_kernel, dim3(gridAll), dim3(kGrokBlock), 0, st, n, d_pattern, tried, from, nmatch);
    // which Match entries' required literals each value contains: one pass for the whole list
    const uint32_t* literalIndex = nullptr;
    {
        int rc = grokLiteralIndex(patterns, state, dev, &literalIndex);
        if (rc != LC_OK) return rc;
    }
    std::vector<uint32_t> carriers;  // per entry: values of the batch that carry its literal (empty: no index)
    if (literalIndex) {
        HIP_TRY(hipMemsetAsync(perPattern, 0, 256, st));
        hipLaunchKernelGGL(grok_literal_index_kernel, dim3(gridAll), dim3(kGrokBlock), 0, st, d_data, d_off, d_len, n, literalIndex,
                           masks, uint32_t(patterns.size()), perPattern, static_cast<const uint32_t*>(nullptr));
        carriers.resize(64);
        HIP_TRY(hipMemcpyAsync(carriers.data(), perPattern, 256, hipMemcpyDeviceToHost, st));
        HIP_TRY(syncCounted(st));
    }
    HIP_TRY(hipMemsetAsync(d_first, 0xFF, size_t(n) * row * 4, st));
    HIP_TRY(hipMemsetAsync(counters, 0, 16, st));

    uint32_t nTried = n;
    uint32_t host[4] = {0, 0, 0, 0};
    // LC_GROK_TRACE=1: one stderr line per Match entry -- values tried / with the literal / past the screen, then (values, ms)
    // per search round (the host waits for a counter after every step anyway, so the clock reads are exact)
    static const bool trace = getenv("LC_GROK_TRACE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto msSince = [&](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(now() - t0).count();
    };
    for (size_t p = 0; p < patterns.size() && nTried; ++p) {
        const GrokDevicePattern& gp = patterns[p];
        // no value of the batch carries this entry's literal: it cannot match anything, and an entry that matches nothing
        // leaves every list as it is
        if (!carriers.empty() && carriers[p] == 0) continue;
        auto tPattern = now();
        std::string traceLine;
        if (trace) traceLine = "grok[" + std::to_string(p) + "] engine " + std::to_string(gp.re->engine) + " tried " + std::to_string(nTried);
        const uint32_t* in = tried;  // round 0 searches every value still undecided, from its first byte ...
        uint32_t nIn = nTried;
        uint32_t* outs[2] = {roundIn, roundOut};
        int flip = 0;
        if (!gp.re->requiredLiteral.empty()) {  // ... that contains the literal every match of this pattern must contain
            GrokLiteral lit;
            const std::string& s = gp.re->requiredLiteral;
            lit.len = uint32_t(std::min<size_t>(s.size(), sizeof lit.bytes));
            std::memcpy(lit.bytes, s.data() + (s.size() - lit.len), lit.len);
            const uint32_t perBlock = kGrokBlock / 64;
            if (literalIndex)
                hipLaunchKernelGGL(grok_mask_filter_kernel, dim3((nTried + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st, tried,
                                   nTried, masks, uint32_t(p), outs[1], counters);
            else
                hipLaunchKernelGGL(grok_literal_filter_kernel, dim3((nTried + perBlock - 1) / perBlock), dim3(kGrokBlock), 0, st,
                                   tried, nTried, d_data, d_off, d_len, lit, outs[1], counters);
            HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(syncCounted(st));
            nIn = host[0];
            in = outs[1];
            HIP_TRY(hipMemsetAsync(counters, 0, 4, st));
            if (trace) traceLine += " literal " + std::to_string(nIn) + " (" + std::to_string(msSince(tPattern)).substr(0, 6) + " ms)";
        }
        // ... and a match of the pattern's prefix, then of the relaxed whole pattern (fast TDFA kernel, status only)
        // (the relaxed screen rejects nearly everything the prefix screen rejects, and each pass costs a launch and a counter read,
        // ~0.25 ms: the prefix screen only goes first where it saves the relaxed one a large candidate set -- LC_GROK_PREFIX_ABOVE)
        const uint32_t prefixAbove = opts.prefixScreenAbove;
        for (lc_regex* scr : {gp.screen, gp.relaxed}) {
            if (!scr || !nIn) continue;
            if (scr == gp.screen && gp.relaxed && nIn <= prefixAbove) continue;
            uint32_t* out = in == outs[0] ? outs[1] : outs[0];
            if (!scr->hasTdfa && !scr->screenBlob.empty()) {  // a plain DFA with its table in L2: screens and filters in one kernel
                int rc = lcScreenOnStream(scr, {.d_data = d_data, .d_off = d_off, .d_len = d_len, .n = nIn, .d_order = in, .dev = dev, .stream = st},
                                          out, counters);
                if (rc != LC_OK) return rc;
            } else {
                int rc = lcMatchOnStream(scr, LC_ENGINE_TDFA,
                                         {.d_data = d_data, .d_off = d_off, .d_len = d_len, .n = nIn,
                                          .d_order = in,
                                          .d_caps = caps, .d_status = status, .dev = dev, .stream = st});
                if (rc != LC_OK) return rc;
                hipLaunchKernelGGL(grok_status_filter_kernel, dim3((nIn + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st,
                                   in, nIn, status, out, counters);
            }
            HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(syncCounted(st));
            nIn = host[0];
            in = out;
            flip = in == outs[0] ? 1 : 0;
            HIP_TRY(hipMemsetAsync(counters, 0, 4, st));
            if (trace)
                traceLine += std::string(scr == gp.screen ? " screen " : " relaxed ") + std::to_string(nIn) + " (" +
                             std::to_string(msSince(tPattern)).substr(0, 6) + " ms)";
        }
        // the match kernels write this pattern's own groups only (whole match + its columns), not the widest pattern's row
        const uint32_t capsRow = 2 * (gp.columns + 1);
        // one search round over the values listed in `list`: the pattern's kernel, then grok_advance_kernel (matches recorded,
        // values that stay in play appended to `out`, their number added to counters[0])
        auto searchRound = [&](lc_regex* re, const uint32_t* list, uint32_t nList, const uint32_t* resume, uint32_t* out) -> int {
            int rc = lcMatchOnStream(re, re->engine,
                                     {.d_data = d_data, .d_off = d_off, .d_len = d_len, .n = nList,
                                      .d_order = list,
                                      .d_resume = resume,
                                      .ngroups = capsRow / 2, .d_caps = caps, .d_status = status, .dev = dev, .stream = st});
            if (rc != LC_OK) return rc;
            hipLaunchKernelGGL(grok_advance_kernel, dim3((nList + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st, list, nList,
                               status, caps, capsRow, row, gp.columns, d_len, from, nmatch, d_pattern, d_first, d_extra, extraCap, out,
                               counters);
            return LC_OK;
        };
        if (gp.anchored && nIn) {
            // Round 0 searches every value from its first byte, and a log format matches FROM the first byte: the anchored search
            // (a tagged DFA, tables in L2, one value per lane) finds exactly what the search would find whenever the search's
            // leftmost match starts at byte 0; the values it does not match go to the search proper (their match, if any, starts
            // later).  Both append to the same next-round list.
            auto tRound = now();
            uint32_t* out = outs[flip];
            int rc = lcMatchOnStream(gp.anchored, gp.anchored->engine,
                                     {.d_data = d_data, .d_off = d_off, .d_len = d_len, .n = nIn,
                                      .d_order = in,
                                      .ngroups = capsRow / 2, .d_caps = caps, .d_status = status, .dev = dev, .stream = st});
            if (rc != LC_OK) return rc;
            hipLaunchKernelGGL(grok_unmatched_kernel, dim3((nIn + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st, in, nIn, status,
                               unanchored, counters + 3);
            hipLaunchKernelGGL(grok_advance_kernel, dim3((nIn + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st, in, nIn, status,
                               caps, capsRow, row, gp.columns, d_len, from, nmatch, d_pattern, d_first, d_extra, extraCap, out, counters);
            HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(syncCounted(st));
            const uint32_t nRest = host[3];
            HIP_TRY(hipMemsetAsync(counters + 3, 0, 4, st));
            if (trace)
                traceLine += " anchored " + std::to_string(nIn) + " -> rest " + std::to_string(nRest) + " (" +
                             std::to_string(msSince(tRound)).substr(0, 7) + " ms)";
            if (nRest) {
                auto tRest = now();
                rc = searchRound(gp.re, unanchored, nRest, from, out);
                if (rc != LC_OK) return rc;
                HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
                HIP_TRY(syncCounted(st));
                if (trace) traceLine += " round " + std::to_string(nRest) + " (" + std::to_string(msSince(tRest)).substr(0, 7) + " ms)";
            }
            nIn = host[0];
            in = out;
            flip ^= 1;
            HIP_TRY(hipMemsetAsync(counters, 0, 4, st));
        }
        while (nIn) {
            auto tRound = now();
            const uint32_t roundValues = nIn;
            uint32_t* out = outs[flip];
            int rc = searchRound(gp.re, in, nIn, from, out);
            if (rc != LC_OK) return rc;
            HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(syncCounted(st));
            nIn = host[0];
            in = out;
            flip ^= 1;
            HIP_TRY(hipMemsetAsync(counters, 0, 4, st));  // counters[0] only; the extra-row count keeps running
            if (trace) traceLine += " round " + std::to_string(roundValues) + " (" + std::to_string(msSince(tRound)).substr(0, 7) + " ms)";
        }
        hipLaunchKernelGGL(grok_finish_kernel, dim3((nTried + kGrokBlock - 1) / kGrokBlock), dim3(kGrokBlock), 0, st, tried,
                           nTried, int32_t(p), nmatch, d_pattern, from, next, counters);
        HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(syncCounted(st));
        if (trace) fprintf(stderr, "%s settled %u total %.3f ms\n", traceLine.c_str(), nTried - host[2], msSince(tPattern));
        nTried = host[2];
        std::swap(tried, next);
        HIP_TRY(hipMemsetAsync(counters + 2, 0, 4, st));
    }
    HIP_TRY(hipMemcpyAsync(d_nextra, counters + 1, 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(syncCounted(st));
    HIP_TRY(hipGetLastError());
    if (host[1] > extraCap) {
        lcSetLastError("grok: " + std::to_string(host[1]) + " extra match rows needed, buffer holds " + std::to_string(extraCap));
        return LC_ERR_OVERFLOW;
    }
    return LC_OK;
}


// ------------------------------------------------------------------------------------------------ speculative path
namespace {
constexpr int kGrokMaxStreams = 16;  // (LC_GROK_STREAMS; the default stays opts.streams = 8)
constexpr uint32_t kGrokScreenStageMax = 44 * 1024;  // a screen's accept flags + table are staged into LDS up to this size
constexpr uint32_t kGrokScreenBigMax = 150 * 1024;   // screens above the first size and up to this one lead the screen table (its order since round 5)
constexpr uint32_t kGrokMaxRounds = GC_BOUND - GC_ROUND0 - 1;  // search rounds that can be queued ahead per entry
constexpr uint32_t kGrokSmallBatch = 262144;  // up to here phase 1 takes the chunk-parallel literal pass and LDS-staged screens, one value per
                                              // lane (round 5: measured better than the lane-per-value passes at 64 Ki (9.3 -> 7.3 ms), 128 Ki
                                              // (14.0 -> 12.1) and 256 Ki values (21.6 -> 20.6); round 4 drew the line at 32 Ki)
constexpr uint32_t kGrokWideFirstBatch = 32768;  // ... and up to here a batch waits for its longest value: wide first pays (16 Ki: -0.3 ms; 64 Ki: +0.5 ms)

// Pinned host words of a thread: what the two syncs of a batch read back.
// (HW_CAND | HW_FIRST | HW_SHADOW mirror the device block dPlanWords: one copy brings all three)
enum { HW_CAND = 0, HW_FIRST = 64, HW_SHADOW = 128, HW_TAIL = 128 + 64 * 64, HW_CNT = 192 + 64 * 64,
       HW_WORDS = 192 + 64 * 64 + 64 * GC_WORDS };
constexpr uint32_t kPlanWords = 64 + 64 + 64 * 64;  // device: candidates per entry | first-candidate counts | who shadows whom
// device tail words (scratch `counters`): [0] gate  [1] xcount (extra rows wanted in xtmp)
// [16] a copy of the caller's nextra word (grok_commit_extra_kernel counts into both)
enum { TW_GATE = 0, TW_XCOUNT = 1, TW_WORDS = 16, TW_NEXTRA = 16 };
static_assert(HW_CNT - HW_TAIL == 64, "hostWords[HW_TAIL ..] mirrors the device block dTail | dCnt");

constexpr size_t kEntryBlockBytes = 64 * sizeof(GrokEntryDev) + 64 * sizeof(GrokScreenDev);

struct PlanThread {
    int device = -1;
    hipStream_t workers[kGrokMaxStreams] = {};
    hipEvent_t fork = nullptr, join[kGrokMaxStreams] = {};
    hipEvent_t tick[2 * 64 + 2 * 64] = {};  // calibration batches: [2a begin/end per entry | 2c begin/end per entry], created on first use
    uint32_t* hostWords = nullptr;        // pinned, HW_*
    // (round 6: the entry table and the remainder screens are ONE pinned block and ONE device block -- one copy per batch;
    // the tail words and the entries' counters likewise, mirrored by hostWords[HW_TAIL ..] -- one copy back per host synchronisation)
    GrokEntryDev* hostEntries = nullptr;  // pinned [64], then hostRemScreens
    GrokEntryDev* dEntries = nullptr;     // device [64], then dRemScreens
    uint32_t* dTail = nullptr;            // device [64] tail words (TW_*), then dCnt
    uint32_t* dCnt = nullptr;             // device [64][GC_WORDS] (inside dTail's block)
    GrokScreenDev* hostRemScreens = nullptr;  // pinned [64]: per ACTIVE entry, its screen (blob == nullptr: none)
    GrokScreenDev* dRemScreens = nullptr;     // device [64]
    uint32_t* dPlanWords = nullptr;           // device [kPlanWords]: perEntry[64] | firstOf[64] | shadow[64][64] (candidates of entry p whose
                                              // value's first candidate is entry f)
    void* hostJobs = nullptr;                 // pinned / device: the job table of round 0's fused launch (runtime_internal.hpp lcLaunchWaveJobs)
    void* dJobs = nullptr;
    void* arena = nullptr;                // device, grow-only: the per-entry arrays of the batch in flight
    size_t arenaCap = 0;
    ~PlanThread() { release(); }
    void release() {
        if (device >= 0 && lcRuntimeUsable()) {
            int cur = 0;
            const bool haveCur = hipGetDevice(&cur) == hipSuccess;
            if (hipSetDevice(device) == hipSuccess) {
                for (auto& w : workers)
                    if (w) {
                        (void)hipStreamSynchronize(w);
                        (void)hipStreamDestroy(w);
                    }
                if (fork) (void)hipEventDestroy(fork);
                for (auto& e : tick)
                    if (e) (void)hipEventDestroy(e);
                for (auto& e : join)
                    if (e) (void)hipEventDestroy(e);
                if (hostWords) (void)hipHostFree(hostWords);
                if (hostEntries) (void)hipHostFree(hostEntries);
                if (dEntries) (void)hipFree(dEntries);
                if (dTail) (void)hipFree(dTail);
                if (dPlanWords) (void)hipFree(dPlanWords);
                if (hostJobs) (void)hipHostFree(hostJobs);
                if (dJobs) (void)hipFree(dJobs);
                if (arena) (void)hipFree(arena);
            }
            if (haveCur) (void)hipSetDevice(cur);
        }
        for (auto& w : workers) w = nullptr;
        for (auto& e : join) e = nullptr;
        for (auto& e : tick) e = nullptr;
        fork = nullptr;
        hostWords = nullptr;
        hostEntries = nullptr;
        dEntries = nullptr;
        dTail = nullptr;
        dCnt = nullptr;
        hostRemScreens = nullptr;
        dRemScreens = nullptr;
        dPlanWords = nullptr;
        hostJobs = nullptr;
        dJobs = nullptr;
        arena = nullptr;
        arenaCap = 0;
        device = -1;
    }
    int ensure(int dev, uint32_t nStreams) {
        if (device != dev) {
            release();
            lcRegisterExitHook();
            device = dev;
            HIP_TRY(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&hostWords), HW_WORDS * 4, hipHostMallocDefault));
            static_assert((64 * sizeof(GrokEntryDev)) % alignof(GrokScreenDev) == 0, "the remainder screens sit behind the entry table");
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&hostEntries), kEntryBlockBytes, hipHostMallocDefault));
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dEntries), kEntryBlockBytes));
            hostRemScreens = reinterpret_cast<GrokScreenDev*>(hostEntries + 64);
            dRemScreens = reinterpret_cast<GrokScreenDev*>(dEntries + 64);
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dTail), (64 + 64 * GC_WORDS) * 4));
            dCnt = dTail + 64;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dPlanWords), kPlanWords * 4));
            HIP_TRY(hipHostMalloc(&hostJobs, lcWaveJobTableBytes(), hipHostMallocDefault));
            HIP_TRY(hipMalloc(&dJobs, lcWaveJobTableBytes()));
        }
        for (uint32_t s = 0; s < nStreams; ++s)
            if (!workers[s]) {
                HIP_TRY(hipStreamCreateWithFlags(&workers[s], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&join[s], hipEventDisableTiming));
            }
        return LC_OK;
    }
    int ensureArena(size_t bytes) {
        if (arenaCap >= bytes) return LC_OK;
        if (arena) {
            HIP_TRY(hipDeviceSynchronize());  // (a larger batch than ever before: rare; nothing of ours is in flight here anyway)
            (void)hipFree(arena);
            arena = nullptr;
            arenaCap = 0;
        }
        const size_t want = bytes + (bytes >> 2) + (1u << 20);
        HIP_TRY(hipMalloc(&arena, want));
        arenaCap = want;
        return LC_OK;
    }
};
thread_local PlanThread tlsPlan;

// the screen the merged launch walks for an entry: the relaxed whole-pattern screen when there is one (it rejects nearly
// everything the prefix screen rejects), else the prefix screen
lc_regex* planScreenOf(const GrokDevicePattern& gp) {
    // (Round 6 measured the prefix screen in place of a relaxed screen too big for LDS and left it off: DESIGN.md,
    // profiles/round6_grok_steps.txt.)
    if (gp.relaxed && !gp.relaxed->screenBlob.empty()) return gp.relaxed;
    if (gp.screen && !gp.screen->screenBlob.empty()) return gp.screen;
    return nullptr;
}
// bytes of (accept flags + table) the plan stages into LDS for a screen; 0: the table is walked in global memory
uint32_t planScreenLdsBytes(const lc_regex* scr) {
    static const bool noStage = getenv("LC_GROK_SCREEN_NO_LDS") != nullptr;
    const uint32_t stage = scr->screenBlob[SC_TOTAL_BYTES] - scr->screenBlob[SC_OFF_ACCEPT];
    return (!noStage && stage <= kGrokScreenStageMax) ? (stage + 3u) & ~3u : 0u;
}

int grokScreenTable(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, int dev, const GrokScreenDev** table,
                    uint32_t* count, uint32_t* ldsBytes) {
    std::lock_guard<std::mutex> g(state->m);
    if (!state->screensBuilt[dev]) {
        static const bool noStage = getenv("LC_GROK_SCREEN_NO_LDS") != nullptr;
        // (the screens of up to kGrokScreenBigMax that do not fit beside other workgroups go first: the order the table has always had)
        std::vector<GrokScreenDev> host, rest;
        uint32_t maxStage = 0;
        for (size_t p = 0; p < patterns.size(); ++p) {
            lc_regex* scr = planScreenOf(patterns[p]);
            if (!scr) continue;
            GrokScreenDev d{};
            int rc = lcEnsureScreenUploaded(scr, dev, &d.blob);
            if (rc != LC_OK) return rc;
            d.bit = uint32_t(p);
            const uint32_t stage = scr->screenBlob[SC_TOTAL_BYTES] - scr->screenBlob[SC_OFF_ACCEPT];
            d.ldsBytes = planScreenLdsBytes(scr);
            const bool big = !noStage && !d.ldsBytes && stage <= kGrokScreenBigMax;
            maxStage = std::max(maxStage, d.ldsBytes);
            if (getenv("LC_GROK_TRACE"))
                fprintf(stderr, "grok screen of entry %zu: %u states x %u classes, %u bytes (%s)%s; prefix screen %u states\n", p, scr->screenBlob[SC_NSTATES],
                        scr->screenBlob[SC_NCLASSES], stage, d.ldsBytes ? "staged in LDS" : "through L2",
                        scr == patterns[p].relaxed ? " relaxed" : " prefix",
                        (patterns[p].screen && !patterns[p].screen->screenBlob.empty()) ? patterns[p].screen->screenBlob[SC_NSTATES] : 0u);
            (big ? host : rest).push_back(d);
        }
        host.insert(host.end(), rest.begin(), rest.end());
        if (!host.empty()) {
            void* p = nullptr;
            HIP_TRY(hipMalloc(&p, host.size() * sizeof(GrokScreenDev)));
            const hipError_t e = hipMemcpy(p, host.data(), host.size() * sizeof(GrokScreenDev), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(p);
                return lcHipFail(e, "hipMemcpy(screen table)");
            }
            state->dScreens[dev] = p;
        }
        state->nScreens[dev] = uint32_t(host.size());
        state->hostScreens[dev] = host;
        state->screenLdsBytes[dev] = maxStage;
        state->screensBuilt[dev] = true;
    }
    *table = static_cast<const GrokScreenDev*>(state->dScreens[dev]);
    *count = state->nScreens[dev];
    *ldsBytes = state->screenLdsBytes[dev];
    return LC_OK;
}

// ---- phase 1 of the plan: the batch's buffers cleared, the length order, the literal index (or every bit set), all screens, the
// candidate counts -- queued on `st`, nothing read back.  The matcher runs it with stage = 2; lcGrokPlanMasksDevice (introspection for
// tests, include/lc_grok.h) runs the same code and may stop behind the literal pass (stage = 1).  d_first / d_nextra: the matcher's
// outputs, cleared along with everything else (nullptr: none).
struct GrokPhase1 {
    uint32_t *winner = nullptr, *undecided = nullptr, *order = nullptr;  // in the caller's scratch
    uint64_t* masks = nullptr;                                           // likewise
    const uint32_t* literalIndex = nullptr;
    uint32_t nScreens = 0;
    bool small = false;
};
int grokPlanPhase1(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, PlanThread& T, uint32_t row, const uint8_t* d_data,
                   const uint32_t* d_off, const uint32_t* d_len, uint32_t n, int32_t* d_first, uint32_t* d_nextra, void* d_scratch,
                   hipStream_t st, int dev, int stage, GrokPhase1* out) {
    const uint32_t nP = uint32_t(patterns.size());
    // scratch: winner u32[n] | undecided u32[n] from the head, tail words / perEntry / masks at their fixed places
    uint8_t* head = static_cast<uint8_t*>(d_scratch);
    uint32_t* winner = reinterpret_cast<uint32_t*>(head);
    uint32_t* undecided = winner + n;
    uint8_t* tailAt = head + alignUp(size_t(n) * row * 4, 256) + alignUp(n, 256) + 7 * alignUp(size_t(n) * 4, 256);
    uint32_t* perEntry = T.dPlanWords;                               // [64] (then firstOf[64], shadow[64][64]: one block, one copy back)
    uint64_t* masks = reinterpret_cast<uint64_t*>(tailAt + 512);

    const uint32_t gridAll = (n + kGrokPlanBlock - 1) / kGrokPlanBlock;
    // Small batches wait for their LONGEST value (every kernel below is a dependent chain per value): chunk-parallel literal pass,
    // screen tables in LDS.  Large batches are about values in flight and equal work per wavefront: lane-per-value in length order.
    static const uint32_t smallBatch = [] {  // LC_GROK_SMALL_BATCH: A/B measurements
        const char* v = getenv("LC_GROK_SMALL_BATCH");
        return v ? uint32_t(atol(v)) : kGrokSmallBatch;
    }();
    const bool small = n <= smallBatch;
    uint32_t* order = reinterpret_cast<uint32_t*>(head + alignUp(size_t(n) * row * 4, 256) + alignUp(n, 256));
    uint32_t* orderWork = reinterpret_cast<uint32_t*>(tailAt + 512 + alignUp(size_t(n) * 8, 256));  // work words behind the masks
    {   // everything the batch needs cleared, in one launch (round 6: seven hipMemsetAsync calls between the kernels of phase 1)
        GrokInitJobs J{};
        auto fill = [&](void* p, size_t bytes, uint32_t value) {
            J.p[J.n] = static_cast<uint32_t*>(p);
            J.words[J.n] = uint32_t(bytes / 4);
            J.value[J.n] = value;
            ++J.n;
        };
        fill(T.dTail, size_t(64 + 64 * GC_WORDS) * 4, 0u);
        fill(T.dPlanWords, size_t(kPlanWords) * 4, 0u);
        fill(winner, size_t(n) * 8, 0xFFFFFFFFu);
        if (d_first) fill(d_first, size_t(n) * row * 4, 0xFFFFFFFFu);
        if (d_nextra) fill(d_nextra, 4, 0u);
        const uint32_t most = uint32_t(std::max(size_t(n) * 2, size_t(n) * row));
        hipLaunchKernelGGL(grok_init_kernel, dim3(std::min(2048u, (most + kGrokPlanBlock - 1) / kGrokPlanBlock)), dim3(kGrokPlanBlock), 0, st, J);
    }
    {
        int rc = lcLengthOrderOnStream(d_off, d_len, 0, n, orderWork, order, st);
        if (rc != LC_OK) return rc;
    }
    const uint32_t* literalIndex = nullptr;
    {
        int rc = grokLiteralIndex(patterns, state, dev, &literalIndex);
        if (rc != LC_OK) return rc;
    }
    // (round 6) the index's tables in LDS when two workgroups of them fit a CU: grok_literal_lds_kernel.  LC_GROK_LITERAL_LDS=0: through L2.
    const uint32_t litStageBytes = [&]() -> uint32_t {
        const char* v = getenv("LC_GROK_LITERAL_LDS");
        if (!literalIndex || !small || (v && v[0] == '0')) return 0u;
        const uint32_t bytes = uint32_t(state->literalBlob.size() * 4) - state->literalBlob[GL_OFF_MASKS];
        return ((state->literalBlob[GL_OFF_MASKS] & 7u) == 0 && bytes <= 78 * 1024) ? bytes : 0u;
    }();
    if (litStageBytes) {
        if (const int rc = lcAllowLds(reinterpret_cast<const void*>(grok_literal_lds_kernel), dev, litStageBytes); rc != LC_OK) return rc;
        static thread_local uint32_t cus[kLcMaxDevices] = {};
        if (dev < kLcMaxDevices && !cus[dev]) {
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDeviceProperties(&prop, dev));
            cus[dev] = uint32_t(prop.multiProcessorCount);
        }
        const uint32_t slots = 2u * (dev < kLcMaxDevices && cus[dev] ? cus[dev] : 256u);
        lcNoteKernel("grok_literal_lds_kernel");
        const uint32_t quadBlocks = ((n + 3) / 4 + kGrokPlanBlock / 64 - 1) / (kGrokPlanBlock / 64);  // (a wavefront takes four values at a time)
        hipLaunchKernelGGL(grok_literal_lds_kernel, dim3(std::min(slots, quadBlocks)), dim3(kGrokPlanBlock), litStageBytes, st, d_data, d_off, d_len, n,
                           literalIndex, masks, litStageBytes, static_cast<const uint32_t*>(order));
    } else if (literalIndex && small) {
        lcNoteKernel("grok_literal_chunk_kernel");
        hipLaunchKernelGGL(grok_literal_chunk_kernel, dim3((n + kGrokPlanBlock / 64 - 1) / (kGrokPlanBlock / 64)), dim3(kGrokPlanBlock), 0, st,
                           d_data, d_off, d_len, n, literalIndex, masks);
    } else if (literalIndex) {
        lcNoteKernel("grok_literal_index_kernel");
        hipLaunchKernelGGL(grok_literal_index_kernel, dim3(gridAll), dim3(kGrokBlock), 0, st, d_data, d_off, d_len, n, literalIndex, masks,
                           nP, static_cast<uint32_t*>(nullptr), static_cast<const uint32_t*>(order));
    } else {
        lcNoteKernel("grok_mask_fill_kernel");
        hipLaunchKernelGGL(grok_mask_fill_kernel, dim3(gridAll), dim3(kGrokPlanBlock), 0, st, masks, n,
                           nP >= 64 ? ~0ull : ((1ull << nP) - 1ull));
    }
    out->winner = winner;
    out->undecided = undecided;
    out->order = order;
    out->masks = masks;
    out->literalIndex = literalIndex;
    out->small = small;
    if (stage == 1) {
        HIP_TRY(hipGetLastError());
        return LC_OK;
    }
    const GrokScreenDev* screens = nullptr;
    uint32_t nScreens = 0, screenLds = 0;
    {
        int rc = grokScreenTable(patterns, state, dev, &screens, &nScreens, &screenLds);
        if (rc != LC_OK) return rc;
    }
    if (nScreens) {
        // slices: short enough that a small batch still spreads over the chip, long enough that the table staging is amortised
        uint32_t sliceLen = ((n / 64 + 255) / 256) * 256;
        sliceLen = std::max(256u, std::min(small ? 4096u : 1024u, sliceLen));
        // (round 5) small batches: never more than one value per lane -- the slices are in length order, the first one holds the 4 KiB
        // values, and a screen that half of them carry walked two of them per lane, one after the other
        if (small) sliceLen = 256u;
        // (round 6) staged tables are staged SCALED (grok_plan_kernel.hpp grokScreenWalkScaled); LC_GROK_SCREEN_SCALED=0: as before
        const uint32_t screenWalk = [] {
            const char* v = getenv("LC_GROK_SCREEN_SCALED");
            return (v && v[0] == '0') ? 0u : 32u;
        }();
        const uint32_t slices = (n + sliceLen - 1) / sliceLen;
        lcNoteKernel("grok_screen_all_kernel");
        static const bool splitScreens = getenv("LC_GROK_SCREEN_SPLIT") != nullptr;  // diagnosis: one launch per screen (a kernel trace then times each)
        if (splitScreens) {
            for (uint32_t k = 0; k < nScreens; ++k)
                hipLaunchKernelGGL(grok_screen_all_kernel, dim3(slices, 1), dim3(kGrokPlanBlock), size_t(sliceLen) * 4 + (small ? screenLds : 0), st,
                                   d_data, d_off, d_len, n, sliceLen, screens + k, reinterpret_cast<unsigned long long*>(masks),
                                   static_cast<const uint32_t*>(order), (small ? 1u : 0u) | screenWalk);
        } else {
            // (grid (screens, slices): the slices of the longest values first -- grok_plan_kernel.hpp; LC_GROK_SCREEN_TRANSPOSED=0: as before)
            const char* tv = getenv("LC_GROK_SCREEN_TRANSPOSED");
            const bool transposed = !(tv && tv[0] == '0') && slices <= 65535u;
            hipLaunchKernelGGL(grok_screen_all_kernel, transposed ? dim3(nScreens, slices) : dim3(slices, nScreens), dim3(kGrokPlanBlock),
                               size_t(sliceLen) * 4 + (small ? screenLds : 0), st, d_data, d_off, d_len, n, sliceLen, screens,
                               reinterpret_cast<unsigned long long*>(masks), static_cast<const uint32_t*>(order),
                               (small ? 1u : 0u) | screenWalk | (transposed ? 128u : 0u));
        }
    }
    uint32_t* firstOf = T.dPlanWords + 64;   // [64]
    uint32_t* shadowBy = T.dPlanWords + 128;  // [64][64]
    lcNoteKernel("grok_count_kernel");
    hipLaunchKernelGGL(grok_count_kernel, dim3(gridAll), dim3(kGrokPlanBlock), 0, st, masks, n, nP, perEntry, firstOf, shadowBy);
    HIP_TRY(hipGetLastError());
    out->nScreens = nScreens;
    return LC_OK;
}

static_assert(grokplan::CW_UNANCHORED == GC_UNANCHORED && grokplan::CW_ROUND0 == GC_ROUND0 && grokplan::CW_BOUND == GC_BOUND &&
                  grokplan::CW_WIDE == GC_WIDE && grokplan::CW_OVERFLOW == GC_OVERFLOW && grokplan::CW_REMAINDER == GC_REMAINDER &&
                  grokplan::CW_FILTERED == GC_FILTERED && grokplan::CW_WORDS == GC_WORDS,
              "grok_plan_host.hpp names the counter words of grok_plan_kernel.hpp");
static_assert(HW_FIRST - HW_CAND == grokplan::PW_FIRST && HW_SHADOW - HW_CAND == grokplan::PW_SHADOW && kPlanWords == grokplan::PW_WORDS &&
                  kGrokMaxRounds == grokplan::kMaxRounds && uint32_t(kGrokMaxStreams) == grokplan::kMaxStreams,
              "grok_plan_host.hpp reads the plan words as phase 1 lays them out");

// host view of one active entry of the batch: the planner's part (grok_plan_host.hpp), then the entry's arrays
struct PlanEntry : grokplan::Entry {
    uint32_t capsRow = 0, columns = 0;
    uint32_t ran = 0;        // rounds the entry ran, when it had to go on behind the ones queued for it
    bool wideFirst = false;  // round 0 ran nfa_wide_kernel over every candidate (the entry's history says its values overflow 64 threads)
    uint32_t seq0 = 0;       // launch sequence of round 0's first-chance kernel (lcMatchSecondChanceOnStream)
    uint32_t seqS = 0;       // ... and of the search proper's
    const GrokScreenDev* remainderScreen = nullptr;  // the entry's screen (host copy), walked over what is left behind a first match
    GrokEntryDev dev{};      // the entry's row of the device table; its arrays lie in the thread's arena
    uint32_t* listB = nullptr;
    int32_t* caps = nullptr;
    uint8_t* status = nullptr;
};

// The knobs of the speculative path, read in ONE place.  Per batch -- the GPU tests flip them between batches of one process --
// except the three at the end.
grokplan::Knobs grokReadKnobs() {
    auto text = [](const char* name) { return getenv(name); };
    auto num = [&](const char* name, int dflt) { return text(name) ? atoi(text(name)) : dflt; };
    grokplan::Knobs k;
    k.wideFirst = num("LC_GROK_WIDE_FIRST", 1);
    k.earlyRounds = num("LC_GROK_EARLY_ROUNDS", 1);
    k.flat = !(text("LC_GROK_FLAT") && text("LC_GROK_FLAT")[0] == '0');
    k.remainderLiteral = num("LC_GROK_REMAINDER_LITERAL", 1) != 0;
    k.remainderWon = num("LC_GROK_REMAINDER_WON", 1) != 0;
    k.screenScaled = num("LC_GROK_SCREEN_SCALED", 1) != 0;
    k.fusedStage = text("LC_GROK_FUSED_STAGE") ? (num("LC_GROK_FUSED_STAGE", 0) != 0 ? 1 : 0) : -1;
    static const uint32_t streams = uint32_t(num("LC_GROK_STREAMS", 0));  // overrides the handle's option (A/B measurements)
    static const bool trace = text("LC_GROK_TRACE") != nullptr;
    static const bool remSplit = text("LC_GROK_REM_SPLIT") != nullptr;  // diagnosis: one launch pair per entry (a kernel trace then times each)
    k.streams = streams;
    k.trace = trace;
    k.remSplit = remSplit;
    return k;
}

// One batch on the speculative path: what the call was given, the thread's resources, the plan, and one method per phase.
// grokMatchSpeculative (below) is the sequence of the phases.
struct GrokBatch {
    // ---- the call (the arguments of grokMatchSpeculative, in their order)
    const std::vector<GrokDevicePattern>& patterns;
    GrokDeviceState* state;
    const GrokOptions& opts;
    uint32_t row;
    const uint8_t* d_data;
    const uint32_t *d_off, *d_len;
    uint32_t n;
    int32_t *d_pattern, *d_first, *d_extra;
    uint32_t extraCap;
    uint32_t* d_nextra;
    void* d_scratch;
    hipStream_t st;
    int dev;
    // ---- the thread's resources, the knobs, the plan
    PlanThread& T = tlsPlan;
    GrokBatchStats& stats = tlsStats;
    const grokplan::Knobs K = grokReadKnobs();
    uint32_t nStreams = 1, used = 1;  // worker streams allowed / in use (min(nStreams, nAct))
    GrokPhase1 P1;
    uint32_t *winner = nullptr, *undecided = nullptr;
    const uint32_t *remLiteral = nullptr, *remWinner = nullptr;  // what grok_remainder_literal_kernel gets (both nullptr: it is not launched)
    std::vector<PlanEntry> act;  // the active entries, in the order of the device table
    uint32_t nAct = 0, nSecond = 0, maxCand = 0;
    GrokSlotMap map;
    int32_t* xtmp = nullptr;  // extra rows wanted: [xcap][xstride], at the head of the arena
    uint32_t xcap = 0, xstride = 0;
    uint32_t *gate = nullptr, *xcount = nullptr;
    bool calibrate = false;      // a calibration batch: the entries' launches are timed with events
    bool aheadLaunched = false;  // the remainder screens went out ahead of sync 2
    uint8_t order1[grokplan::kMaxEntries] = {};  // the leftovers deal's order: the chains are queued in it
    grokplan::Chains chains;
    // (round 6) A worker stream waits for the fork when it first GETS work (W), and only the streams that got any are joined: a
    // phase forks into sixteen streams and usually uses three, and the thirteen idle ones cost the host 26 calls per fork / join
    // and the batch's stream thirteen barrier packets that it works through one after the other (0.09 ms between the end of round
    // 0 and the first kernel behind the join, profiles/round6_grok_timeline.txt).
    uint32_t waitedMask = 0, touchedMask = 0;
    std::chrono::steady_clock::time_point t0;
    double tPhase1 = 0, tPhase3 = 0;

    double msNow() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    uint32_t cnt(size_t a, uint32_t word) const { return T.hostWords[HW_CNT + a * GC_WORDS + word]; }
    static uint32_t grid(uint32_t slots) { return (slots + kGrokPlanBlock - 1) / kGrokPlanBlock; }          // a lane per slot
    static uint32_t waveGrid(uint32_t slots) { return (slots + kGrokPlanBlock / 64 - 1) / (kGrokPlanBlock / 64); }  // a wavefront per slot
    lc_regex* firstOf(const PlanEntry& e) const { return patterns[e.p].anchored ? patterns[e.p].anchored : patterns[e.p].re; }  // round 0's automaton

    int fork() {
        HIP_TRY(hipEventRecord(T.fork, st));
        waitedMask = 0;  // (everybody waits for THIS fork from now on; what was touched before stays to be joined)
        return LC_OK;
    }
    hipStream_t W(int s) {  // (a failure surfaces at the join: hipGetLastError)
        const uint32_t bit = 1u << uint32_t(s);
        if (!(waitedMask & bit)) {
            (void)hipStreamWaitEvent(T.workers[s], T.fork, 0);
            waitedMask |= bit;
        }
        touchedMask |= bit;
        return T.workers[s];
    }
    int join(int rc) {
        lcSetDecideSlot(0);
        if (rc == LC_OK && hipGetLastError() != hipSuccess) rc = lcHipFail(hipGetLastError(), "grok entry launch");
        if (rc != LC_OK) {
            for (uint32_t s = 0; s < used; ++s) (void)hipStreamSynchronize(T.workers[s]);
            return rc;
        }
        for (uint32_t s = 0; s < used; ++s) {
            if (!((touchedMask >> s) & 1u)) continue;
            HIP_TRY(hipEventRecord(T.join[s], T.workers[s]));
            HIP_TRY(hipStreamWaitEvent(st, T.join[s], 0));
        }
        touchedMask = 0;
        return LC_OK;
    }
    // entry e's candidates as a launch sees them: `bound` of them at most, the count on the device, the list and the resume offsets
    MatchBatch entryBatch(const PlanEntry& e, uint32_t bound, const uint32_t* count, const uint32_t* list, const uint32_t* resume, hipStream_t ws) const {
        return MatchBatch{.d_data = d_data, .d_off = e.dev.off, .d_len = e.dev.len, .n = bound,
                          .d_n = count,
                          .d_order = list,
                          .d_resume = resume,
                          .ngroups = e.capsRow / 2, .d_caps = e.caps, .d_status = e.status, .dev = dev, .stream = ws};
    }
    // An entry whose values needed more than 64 threads in recent batches (GC_WIDE, noted behind the batch) goes WIDE FIRST: its
    // first chance is nfa_wide_kernel over every candidate, and what is left behind it are the decide kernels alone.  Round 4's
    // timeline: the longest entry's first chance 1.0 ms + its second chance (14 values restarted from byte 0) 1.1 ms, back to back
    // on the critical path of the batch; now 1.1 ms.
    bool wantsWideFirst(lc_regex* h) const {
        if (!K.wideFirst || h->engine != LC_ENGINE_NFA || !lcNfaWideApplies(h)) return false;
        if (K.wideFirst >= 2) return true;
        return n <= kGrokWideFirstBatch && h->grokOverflowSeen.load(std::memory_order_relaxed) != 0;
    }
    // one engine call of entry e on stream ws: the first-chance kernel ...
    int runFirst(PlanEntry& e, lc_regex* h, bool wide, const uint32_t* count, const uint32_t* list, bool withFrom, uint32_t* seq, hipStream_t ws) {
        const MatchBatch b = entryBatch(e, e.cand, count, list, withFrom ? e.dev.from : nullptr, ws);
        if (wide) return lcMatchWideFirstOnStream(0, h, h->engine, b, seq, e.dev.cnt + GC_WIDE);
        return lcMatchFirstOnStream(h, h->engine, b, seq);
    }
    // ... and what is left behind it (note: the entry's GC_WIDE word, set when the wide kernel had anything to do)
    int runSecond(PlanEntry& e, lc_regex* h, bool wide, const uint32_t* count, const uint32_t* list, bool withFrom, uint32_t seq, uint32_t* note,
                  hipStream_t ws) {
        const MatchBatch b = entryBatch(e, e.cand, count, list, withFrom ? e.dev.from : nullptr, ws);
        if (wide) return lcMatchWideFirstOnStream(1, h, h->engine, b, &seq, nullptr);
        lcSetWideNote(note);
        const int r = lcMatchSecondChanceOnStream(h, h->engine, b, seq);
        lcSetWideNote(nullptr);
        return r;
    }
    // grok_post_kernel over `rows` entries of the table from `first` on (most: the largest of them): overflowed slots -> the entry's
    // overflow list, slots the anchored search did not match -> its unanchored list, matches recorded, what is still in play -> listA
    void post(hipStream_t ws, size_t first, size_t rows, uint32_t most, const uint32_t* in, const uint32_t* inCount, uint32_t flags,
              unsigned long long skip) {
        hipLaunchKernelGGL(grok_post_kernel, dim3(grid(most), uint32_t(rows)), dim3(kGrokPlanBlock), 0, ws, T.dEntries, uint32_t(first), in, inCount,
                           flags, xtmp, xcap, xstride, xcount, skip);
    }
    // the values won so far (atomicMin per value: idempotent, the finish runs it again); one: that entry's alone
    void wonSoFar(hipStream_t ws, uint32_t most, uint32_t rows, uint32_t one) {
        hipLaunchKernelGGL(grok_entry_finish_kernel, dim3(grid(most), rows), dim3(kGrokPlanBlock), 0, ws, T.dEntries, winner, undecided,
                           static_cast<const uint32_t*>(nullptr), one);
    }
    // The remainder screens of `rows` entries of the table from `first` on: the literal index over the remainders (and the slots of
    // values an earlier entry has won dropped), then the entries' screens; the survivors are counted onto the gate word.  The other
    // entries' workgroups leave at once (skip mask).  ahead: queued before the host has read round 0's counts -- the kernels test the
    // entry's overflow / unanchored counts themselves.
    void remainderScreens(hipStream_t ws, size_t first, uint32_t rows, uint32_t most, uint32_t lds, unsigned long long skip, bool ahead) {
        const GrokEntryDev* entries = static_cast<const GrokEntryDev*>(T.dEntries) + first;
        const uint32_t walk = (P1.small ? 1u : 0u) | (K.screenScaled ? 32u : 0u) | (ahead ? 64u : 0u);
        if (remLiteral || remWinner) {
            lcNoteKernel("grok_remainder_literal_kernel");
            hipLaunchKernelGGL(grok_remainder_literal_kernel, dim3(waveGrid(most), rows), dim3(kGrokPlanBlock), 0, ws, d_data, entries, remLiteral, skip,
                               remWinner, ahead ? 1u : 0u);
        }
        lcNoteKernel("grok_remainder_all_kernel");
        hipLaunchKernelGGL(grok_remainder_all_kernel, dim3(grid(most), rows), dim3(kGrokPlanBlock), P1.small ? lds : 0, ws, d_data, entries,
                           static_cast<const GrokScreenDev*>(T.dRemScreens) + first, walk, skip, gate);
    }
    void learn(std::atomic<uint32_t>& slot, hipEvent_t b, hipEvent_t e2, uint32_t cand) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, b, e2) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        const uint32_t ns = uint32_t(std::min(4.0e9, std::max(1.0, double(ms) * 1e6 / std::max(1u, cand))));
        const uint32_t old = slot.load(std::memory_order_relaxed);
        slot.store(old ? (old + ns) / 2 : ns, std::memory_order_relaxed);
    }

    // ---- phase 1: length order, literal index, all screens, candidate counts (grokPlanPhase1) -> host (sync 1)
    int phase1() {
        nStreams = std::max(1u, std::min<uint32_t>(K.streams ? K.streams : opts.streams, kGrokMaxStreams));
        if (const int rc = T.ensure(dev, nStreams); rc != LC_OK) return rc;
        t0 = std::chrono::steady_clock::now();
        if (const int rc = grokPlanPhase1(patterns, state, T, row, d_data, d_off, d_len, n, d_first, d_nextra, d_scratch, st, dev, 2, &P1); rc != LC_OK)
            return rc;
        winner = P1.winner;
        undecided = P1.undecided;
        remLiteral = K.remainderLiteral ? P1.literalIndex : nullptr;
        remWinner = K.remainderWon ? winner : nullptr;
        gate = T.dTail + TW_GATE;  // TW_* (the entries' counters behind them: one block, one copy back)
        xcount = T.dTail + TW_XCOUNT;
        HIP_TRY(hipMemcpyAsync(T.hostWords + HW_CAND, T.dPlanWords, size_t(kPlanWords) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(syncCounted(st));  // sync 1: candidates per entry
        tPhase1 = msNow();
        return LC_OK;
    }

    // the entry's arrays, carved from the arena at `at` (arena == nullptr: only counted)
    static void carveEntry(PlanEntry& e, uint8_t* arena, size_t& at) {
        auto take = [&](size_t bytes) {
            uint8_t* p = arena ? arena + at : nullptr;
            at += alignUp(bytes, 256);
            return p;
        };
        auto slots = [&] { return reinterpret_cast<uint32_t*>(take(size_t(e.cand) * 4)); };
        e.dev.off = slots();
        e.dev.len = slots();
        e.dev.line = slots();
        e.dev.from = slots();
        e.dev.nmatch = slots();
        e.dev.listA = slots();
        e.listB = slots();
        e.dev.unanchored = slots();
        e.dev.ovList = slots();
        e.dev.first = reinterpret_cast<int32_t*>(take(size_t(e.cand) * e.capsRow * 4));
        e.dev.caps = e.caps = reinterpret_cast<int32_t*>(take(size_t(e.cand) * e.capsRow * 4));
        e.dev.status = e.status = take(size_t(e.cand) + 16);
    }
    // what the planner is told about list entry p with c candidates, and what the launches need of it
    PlanEntry describe(uint32_t p, uint32_t c) const {
        const GrokDevicePattern& gp = patterns[p];
        PlanEntry e;
        e.p = p;
        e.cand = c;
        e.columns = gp.columns;
        e.capsRow = 2 * (gp.columns + 1);
        // (round 0 is a phase of its own; round 1 reads the screened list)
        e.rounds = std::max(2u, std::min(kGrokMaxRounds, gp.re->grokRounds.load(std::memory_order_relaxed)));
        for (const GrokScreenDev& sd : state->hostScreens[dev])
            if (sd.bit == p) e.remainderScreen = &sd;
        const lc_regex* first = gp.anchored ? gp.anchored : gp.re;
        e.anchored = gp.anchored != nullptr;
        e.firstNfa = first->engine == LC_ENGINE_NFA;
        e.reTdfa = gp.re->engine == LC_ENGINE_TDFA;
        e.remainderSeen = gp.re->grokRemainderSeen.load(std::memory_order_relaxed) != 0;
        // round 0 as a table walk: a complete automaton in global memory, or a lazy one (grok_plan_host.hpp assignLevels)
        if (first->engine == LC_ENGINE_TDFA) e.tableWalk = !first->tdfaL2Blob.empty() && (first->preferWave || !first->hasTdfa);
        else e.tableWalk = first->engine == LC_ENGINE_NFA && first->lazyReady.load(std::memory_order_acquire);
        e.cost = double(c) * (gp.re->engine == LC_ENGINE_NFA ? (gp.anchored ? 8.0 : 40.0) : 1.0);
        // (measured, once a calibration batch has run: ns per candidate of round 0 and of the leftovers)
        const uint32_t c0 = gp.re->grokCost0Ns.load(std::memory_order_relaxed), c1 = gp.re->grokCost1Ns.load(std::memory_order_relaxed);
        e.cost0 = c0 ? double(c0) * c : 0.0;
        e.cost1 = c1 ? double(c1) * c : 0.0;
        // an automaton that walks its tables in global memory (tdfa_l2_kernel) takes as long as its LONGEST candidate -- one dependent
        // read per byte, ~0.7 us per byte, 2.8 ms for a 4 KiB line -- on a grid of a few waves: it goes to the head of its stream,
        // where it runs beside everything else, instead of behind the cheap entries (measured: the step's last 2.8 ms were this)
        auto walksGlobalTables = [](const lc_regex* re) { return re && re->engine == LC_ENGINE_TDFA && !re->hasTdfa && !re->tdfaL2Blob.empty(); };
        // (small batches only -- measured 6.36 -> 4.02 ms on 1000 values, 5.67 -> 6.34 ms on 16 Ki: the runtime maps the worker streams
        // onto a few hardware queues, and with thousands of candidates per entry the wide thread-list kernels, not these, are the
        // long poles; sharing half of the streams among these entries was worse for both sizes)
        if (P1.small && (walksGlobalTables(gp.re) || walksGlobalTables(gp.anchored))) e.cost += 1e12;
        return e;
    }
    // ---- the batch's active entries, their levels, their arrays in the arena, the device table; the candidates scattered to them
    int entries() {
        const uint32_t nP = uint32_t(patterns.size());
        xcap = std::max<uint32_t>(extraCap, n / 4 + 1024);
        xstride = row + 3;
        size_t arenaBytes = alignUp(size_t(xcap) * xstride * 4, 256);  // (xtmp at the head)
        const size_t entriesAt = arenaBytes;
        for (uint32_t p = 0; p < nP; ++p) {
            const uint32_t c = T.hostWords[HW_CAND + p];
            if (!c) continue;
            act.push_back(describe(p, c));
            carveEntry(act.back(), nullptr, arenaBytes);
        }
        nAct = uint32_t(act.size());
        used = std::min<uint32_t>(nStreams, nAct);
        stats.activeEntries = nAct;
        if (const int rc = T.ensureArena(arenaBytes); rc != LC_OK) return rc;
        uint8_t* arena = static_cast<uint8_t*>(T.arena);
        xtmp = reinterpret_cast<int32_t*>(arena);
        size_t at = entriesAt;
        for (PlanEntry& e : act) carveEntry(e, arena, at);  // (in list order: the arena's layout does not depend on the levels)
        grokplan::assignLevels(act.data(), nAct, T.hostWords + HW_CAND, K);
        nSecond = grokplan::sortByLevel(act);
        for (auto& a : map.activeOfBit) a = -1;
        for (size_t a = 0; a < nAct; ++a) {
            PlanEntry& e = act[a];
            e.dev.cnt = T.dCnt + a * GC_WORDS;  // (cleared by grok_init_kernel at the start of the batch)
            e.dev.cand = e.cand;
            e.dev.capsRow = e.capsRow;
            e.dev.bit = e.p;
            e.dev.columns = e.columns;
            e.dev.anchored = e.anchored ? 1u : 0u;
            T.hostEntries[a] = e.dev;
            T.hostRemScreens[a] = e.remainderScreen ? *e.remainderScreen : GrokScreenDev{nullptr, e.p, 0u};
            map.activeOfBit[e.p] = int8_t(a);
            maxCand = std::max(maxCand, e.cand);
            stats.pairs += e.cand;
        }
        if (!nAct) return LC_OK;
        // (the entry table and, behind it, the remainder screens: one block)
        HIP_TRY(hipMemcpyAsync(T.dEntries, T.hostEntries, 64 * sizeof(GrokEntryDev) + nAct * sizeof(GrokScreenDev), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(grok_scatter_kernel, dim3(grid(n)), dim3(kGrokPlanBlock), 0, st, P1.masks, n, nP, d_off, d_len, map, T.dEntries,
                           static_cast<const uint32_t*>(P1.order));
        HIP_TRY(hipGetLastError());
        return LC_OK;
    }

    // ---- phase 2 (round 4).  A batch used to queue 14-17 launches per entry -- 560 for the 46 active entries of configs[2] -- most of
    // them over lists that turn out empty, and the host could not queue them as fast as the device finished them (18 us a launch).
    // Now:  round0     ONE launch for the table-walk entries, one each for the others (the engine's main kernel, the anchored search
    //                  where the entry has one), the post step behind each;
    //       ahead      values won so far, bounds of the shadowed entries, remainder screens of the quiet entries;   counts -> host
    //       runChains  only the entries that have any: second chance, search proper, shadowed entries; then the entry's remainder
    //                  screens or its search rounds;
    //       finish     the first contributing entry per value;   survivors of the screens -> host with the results
    //       survivors  only the entries with survivors: the search rounds behind the first match, then the finish again.
    // Calibration batches (the first three of a handle, then every 64th) time every entry's launches with events; the matcher then
    // deals longest-first to the least loaded stream (grok_plan_host.hpp deal).
    // ---- round 0 of the entries of level 0 (the shadowed ones wait for them: runChains)
    int round0() {
        bool allKnown = true;
        for (const PlanEntry& e : act) allKnown = allKnown && e.cost0 > 0;
        const uint32_t seen = patterns[act[0].p].re->grokBatches.fetch_add(1, std::memory_order_relaxed);
        calibrate = !allKnown || seen < 3 || (seen & 63u) == 0;
        if (calibrate)
            for (size_t k = 0; k < 4 * size_t(nAct); ++k)
                if (!T.tick[k]) HIP_TRY(hipEventCreate(&T.tick[k]));
        return round0Launches();
    }
    // Round 6: the entries whose round 0 is a walk of tables in global memory -- a complete tagged DFA, or the LAZY automaton of an
    // entry that does not determinise -- go in ONE launch (tdfa_wave_multi_kernel) with ONE post launch behind it.  Round 0 used to
    // be ~46 kernels of 30-100 us each plus their 46 post kernels, and lasted as long as the host needed to queue them: the last one
    // started 1.4 ms after the first (profiles/round6_grok_timeline_lazy.txt).  LC_GROK_FUSED_ROUND0=0: one launch per entry.
    struct FusedJobs {
        std::vector<TdfaWaveJob> jobs;
        uint32_t blocks = 0, ldsMax = 0;
        size_t lo = 0, hi = 0;  // the first and the last fused entry of the table
    };
    int prepareFused(FusedJobs& F) {
        // (all entries' candidates together are what the ONE launch walks; LC_GROK_FUSED_STAGE=0/1 forces it: A/B)
        const bool stagePrograms = K.fusedStage >= 0 ? K.fusedStage != 0 : stats.pairs <= 32768;
        int rcJob = LC_OK;
        const bool ok = grokplan::selectFused(act.data(), nAct, K, kTdfaWaveMaxJobs, [&](size_t a) {
            PlanEntry& e = act[a];
            TdfaWaveJob j{};
            uint32_t lds = 0, seq = 0;
            if (!lcWaveJobPrepare(firstOf(e), dev, e.cand, stagePrograms, &j, &lds, &seq, &rcJob)) return rcJob != LC_OK ? -1 : 0;
            j.off = e.dev.off;
            j.len = e.dev.len;
            j.resume = e.anchored ? nullptr : e.dev.from;
            j.caps = e.caps;
            j.status = e.status;
            j.n = e.cand;
            j.nGroupsOut = e.capsRow / 2;
            j.firstBlock = F.blocks;
            F.blocks += (e.cand + kTdfaWaveValues - 1) / kTdfaWaveValues;
            F.ldsMax = std::max(F.ldsMax, lds);
            e.seq0 = seq;  // (a lazy automaton's misses are LC_OVERFLOW under this number: the second chance in the entry's chain takes them)
            e.wideFirst = false;
            if (F.jobs.empty()) F.lo = a;
            F.hi = a;
            F.jobs.push_back(j);
            return 1;
        });
        return ok ? LC_OK : rcJob;
    }
    int launchFused(const FusedJobs& F, hipStream_t ws) {
        const int rc = lcLaunchWaveJobs(d_data, F.jobs.data(), uint32_t(F.jobs.size()), F.blocks, F.ldsMax, T.hostJobs, T.dJobs, dev, ws);
        // the post step of the fused entries: ONE launch over their span of the entry table (the entries in between that are not
        // the fused launch's leave at once: skip mask)
        if (rc == LC_OK) {
            unsigned long long skip = 0;
            uint32_t most = 0;
            for (size_t a = F.lo; a <= F.hi; ++a) {
                if (act[a].fused) most = std::max(most, act[a].cand);
                else skip |= 1ull << a;
            }
            post(ws, F.lo, F.hi - F.lo + 1, most, nullptr, nullptr, GP_ANCHORED_PASS, skip);
        }
        if (K.trace) fprintf(stderr, "grok plan 2a: %zu entries in one launch (%u workgroups, %u B of LDS)\n", F.jobs.size(), F.blocks, F.ldsMax);
        return rc;
    }
    // round 0 of an entry that keeps a launch of its own, on its stream, its post step right behind its kernel (round 5: the one post
    // launch for all entries behind the join (0.12 ms) waited for the slowest entry and then stood between it and the host's read of
    // the counts)
    int round0Entry(size_t a) {
        PlanEntry& e = act[a];
        const GrokDevicePattern& gp = patterns[e.p];
        lcSetDecideSlot(1 + e.stream);
        lc_regex* first = firstOf(e);
        e.wideFirst = wantsWideFirst(first);
        int rc = LC_OK;
        // (failures inside the forked region become rc: the workers are always joined)
        if (calibrate && hipEventRecord(T.tick[2 * a], W(e.stream)) != hipSuccess) rc = lcHipFail(hipGetLastError(), "hipEventRecord(calibration)");
        if (rc == LC_OK) rc = runFirst(e, first, e.wideFirst, nullptr, nullptr, !gp.anchored, &e.seq0, W(e.stream));
        if (calibrate) (void)hipEventRecord(T.tick[2 * a + 1], W(e.stream));
        if (rc == LC_OK) post(W(e.stream), a, 1, e.cand, nullptr, nullptr, GP_ANCHORED_PASS, 0ull);
        if (K.trace)
            fprintf(stderr, "grok plan 2a: entry %u cand %u stream %d engine %s%s%s positions %zu slots %d atomic %d | measured round 0 %.3f ms, leftovers %.3f ms\n",
                    e.p, e.cand, e.stream, first->engine == LC_ENGINE_NFA ? "nfa" : first->hasTdfa ? "tdfa-lds" : "tdfa-l2",
                    gp.anchored ? " (anchored)" : "", e.wideFirst ? " (wide first)" : "", first->nfa.positions.size(), first->nfa.slotCount(),
                    first->nfa.atomicCount, e.cost0 * 1e-6, e.cost1 * 1e-6);
        return rc;
    }
    int round0Launches() {
        FusedJobs F;
        if (const int rc = prepareFused(F); rc != LC_OK) return rc;
        bool others = false;
        for (const PlanEntry& e : act) others = others || (!e.level && !e.fused);
        int rc = others ? fork() : LC_OK;
        if (rc != LC_OK) return rc;
        hipStream_t fusedStream = others ? W(0) : st;
        if (!F.jobs.empty()) rc = launchFused(F, fusedStream);
        uint8_t order0[grokplan::kMaxEntries];
        grokplan::deal(act.data(), nAct, used, false, order0);
        for (size_t i = 0; i < nAct && rc == LC_OK && others; ++i)
            if (!act[order0[i]].level && !act[order0[i]].fused) rc = round0Entry(order0[i]);
        if (others) rc = join(rc);
        else if (rc == LC_OK && hipGetLastError() != hipSuccess) rc = lcHipFail(hipGetLastError(), "grok round 0");
        return rc;
    }

    // ---- round 0's results: the values won so far, the bounds, the remainder screens queued ahead; counts -> host (sync 2)
    int ahead() {
        lcNoteKernel("grok_post_kernel");
        // the values won so far, and for the entries of level >= 1 how many of their slots are still open: an entry all of whose
        // candidates an entry of level 0 has won (COMBINEDAPACHELOG behind COMMONAPACHELOG on a corpus without referrers) queues nothing
        // in its chain -- its dozen launches over empty lists were the tail of the phase
        if (nSecond) {
            wonSoFar(st, maxCand, nAct, 0u);
            hipLaunchKernelGGL(grok_bound_kernel, dim3(grid(maxCand), nSecond), dim3(kGrokPlanBlock), 0, st, T.dEntries, nAct - nSecond,
                               static_cast<const uint32_t*>(winner));  // (the table lists the entries by level)
        }
        // (Tried in round 5 and dropped -- profiles/round5_grok_steps.txt: the chains of level 1, and by the entries' history the
        // leftovers of level 0, queued BEFORE the host reads round 0's counts.  The device has them earlier, but a batch is bound by
        // the rate at which the host can queue launches, and the extra, mostly empty chains cost more than the earlier start gained:
        // 16 Ki values 4.76 -> 5.4 ms, 1000 values 3.9 -> 5.2 ms.)
        // (round 6) The remainder screens, AHEAD of the host's read of round 0's counts.  Queued behind it, that launch pair (0.5 ms: a
        // few thousand remainders of up to 4 KiB, one lane each) started 0.16 ms after round 0 had ended: a copy, a host round trip and
        // the host's planning of the chains (profiles/round6_grok_timeline.txt).  Which entries have nothing else to do is a test of
        // two counters the device has: the launch pair goes out now, on a worker stream beside the copy, and leaves the entries with
        // overflowed or unanchored slots (and the shadowed ones, and the ones whose search rounds their history queues ahead: `skip`)
        // to their chains.
        // (whose rounds are queued ahead is decided ONCE per batch -- another runner thread's batch on the same handle may rewrite that
        // history between here and the chains)
        grokplan::decideEarly(act.data(), nAct, K, calibrate);
        struct {
            unsigned long long skip = 0;  // the shadowed entries and the ones whose rounds are queued ahead leave the launch
            uint32_t most = 0;            // the largest entry in it (0: no launch)
        } h;
        uint32_t lds = 0;
        for (size_t a = 0; a < nAct; ++a) {
            if (act[a].level || act[a].early) h.skip |= 1ull << a;
            else {
                h.most = std::max(h.most, act[a].cand);
                if (act[a].remainderScreen) lds = std::max(lds, act[a].remainderScreen->ldsBytes);
            }
        }
        if (h.most) {
            if (!nSecond) wonSoFar(st, maxCand, nAct, 0u);  // (the literal pass drops the slots of values an earlier entry has won)
            if (const int rc = fork(); rc != LC_OK) return rc;
            hipStream_t gs = W(int(used) - 1);
            if (!K.remSplit) remainderScreens(gs, 0, nAct, h.most, lds, h.skip, true);
            for (uint32_t a = 0; a < (K.remSplit ? nAct : 0u); ++a)
                if (!((h.skip >> a) & 1ull)) remainderScreens(gs, 0, nAct, h.most, lds, ~(1ull << a), true);
            aheadLaunched = true;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(T.hostWords + HW_CNT, T.dCnt, size_t(nAct) * GC_WORDS * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(syncCounted(st));  // sync 2
        for (size_t a = 0; a < nAct; ++a) {
            std::atomic<uint32_t>& cost0 = patterns[act[a].p].re->grokCost0Ns;
            if (calibrate && !act[a].level && !act[a].fused) learn(cost0, T.tick[2 * a], T.tick[2 * a + 1], act[a].cand);
            // (an entry of the fused launch has no kernel of its own to time: a nominal cost keeps the handle "known")
            if (act[a].fused && cost0.load(std::memory_order_relaxed) == 0) cost0.store(100, std::memory_order_relaxed);
        }
        return LC_OK;
    }

    // ---- the chains: what round 0 left undone on the entries of level 0 (second chance of overflowed slots; the search proper for
    // what the anchored search did not match -- minus the values an earlier entry has won meanwhile), and, level by level, the shadowed
    // entries on the values nobody before them has won.  grok_plan_host.hpp builds them as steps; this is the only place that turns
    // a step into launches.
    static uint32_t* listOf(const PlanEntry& e, uint8_t sel) {
        uint32_t* const lists[] = {nullptr, e.dev.listA, e.listB, e.dev.unanchored, e.dev.ovList};  // grokplan::ListSel
        return lists[sel];
    }
    void tick(size_t a, int which, int& rc) {
        if (!calibrate || !act[a].busy) return;
        if (hipEventRecord(T.tick[2 * nAct + 2 * a + size_t(which)], W(act[a].stream)) != hipSuccess && rc == LC_OK && which == 0)
            rc = lcHipFail(hipGetLastError(), "hipEventRecord(calibration)");
    }
    void runStep(const grokplan::Step& s, int& rc) {
        using namespace grokplan;
        const size_t a = s.entry;
        PlanEntry& e = act[a];
        if (s.flags & F_TICK_BEGIN) tick(a, 0, rc);
        if (s.flags & F_TICK_END) {
            int ignored = LC_OK;
            tick(a, 1, ignored);
        }
        if (rc != LC_OK || s.kind == S_TICK) return;
        const GrokDevicePattern& gp = patterns[e.p];
        lc_regex* first = firstOf(e);
        hipStream_t ws = W(e.stream);
        uint32_t* list = listOf(e, s.list);
        uint32_t* out = listOf(e, s.out);
        uint32_t* count = e.dev.cnt + s.count;
        if (s.kind != S_FINISH_SHADOWER && s.kind != S_POST && s.kind != S_REMAINDER) lcSetDecideSlot(1 + e.stream);
        switch (s.kind) {
            case S_FINISH_SHADOWER: wonSoFar(ws, act[s.arg].cand, 1, uint32_t(s.arg)); break;
            case S_SECOND_OVERFLOW: rc = runSecond(e, first, e.wideFirst, count, list, !gp.anchored, e.seq0, e.dev.cnt + GC_WIDE, ws); break;
            case S_POST: post(ws, a, 1, e.cand, list, count, GP_ANCHORED_PASS | GP_OVERFLOW_FINAL, 0ull); break;
            case S_SEARCH_FIRST:
                hipLaunchKernelGGL(grok_filter_won_kernel, dim3(grid(e.cand)), dim3(kGrokPlanBlock), 0, ws, e.dev, static_cast<const uint32_t*>(winner),
                                   static_cast<const uint32_t*>(list), static_cast<const uint32_t*>(count), out, e.dev.cnt + GC_FILTERED);
                rc = runFirst(e, gp.re, false, e.dev.cnt + GC_FILTERED, out, true, &e.seqS, ws);
                break;
            case S_SEARCH_SECOND_POST:
                rc = runSecond(e, gp.re, false, count, list, true, e.seqS, nullptr, ws);
                if (rc == LC_OK) post(ws, a, 1, e.cand, list, count, GP_OVERFLOW_FINAL, 0ull);
                break;
            case S_SHADOWED_FIRST:
                hipLaunchKernelGGL(grok_filter_won_kernel, dim3(grid(e.cand)), dim3(kGrokPlanBlock), 0, ws, e.dev, static_cast<const uint32_t*>(winner),
                                   static_cast<const uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr), out, count);
                e.wideFirst = wantsWideFirst(first);
                rc = runFirst(e, first, e.wideFirst, count, out, !gp.anchored, &e.seq0, ws);
                break;
            case S_SHADOWED_SECOND_POST:
                rc = runSecond(e, first, e.wideFirst, count, list, !gp.anchored, e.seq0, e.dev.cnt + GC_WIDE, ws);
                if (rc == LC_OK) post(ws, a, 1, e.cand, list, count, GP_ANCHORED_PASS | GP_OVERFLOW_FINAL, 0ull);
                break;
            case S_ROUND:
                rc = lcMatchOnStream(gp.re, gp.re->engine, entryBatch(e, e.cand, count, list, e.dev.from, ws));
                if (rc != LC_OK) return;
                hipLaunchKernelGGL(grok_advance2_kernel, dim3(grid(e.cand)), dim3(kGrokPlanBlock), 0, ws, static_cast<const uint32_t*>(list), e.cand,
                                   static_cast<const uint32_t*>(count), e.status, e.caps, e.capsRow, e.columns, e.dev, xtmp, xcap, xstride, xcount, out,
                                   e.dev.cnt + GC_ROUND0 + s.arg, (s.flags & F_GATE) ? gate : static_cast<uint32_t*>(nullptr));
                break;
            case S_REMAINDER:  // (grid.y = 1 over a table that begins at this entry)
                remainderScreens(ws, a, 1, e.cand, e.remainderScreen ? e.remainderScreen->ldsBytes : 0u, 0ull, false);
                break;
        }
    }
    void traceChains() const {
        for (size_t i = 0; i < nAct; ++i) {
            const size_t a = order1[i];
            const PlanEntry& e = act[a];
            const char* rounds = e.early ? " + rounds" : "";
            if (e.level && cnt(a, GC_BOUND) == 0)
                fprintf(stderr, "grok plan 2c: entry %u level %u cand %u: every value already won\n", e.p, e.level, e.cand);
            else if (e.level) fprintf(stderr, "grok plan 2c: entry %u level %u cand %u stream %d%s\n", e.p, e.level, e.cand, e.stream, rounds);
            else if (e.busy || e.early)
                fprintf(stderr, "grok plan 2c: entry %u overflowed %u unanchored %u%s\n", e.p, cnt(a, GC_OVERFLOW), cnt(a, GC_UNANCHORED), rounds);
        }
    }
    int runChains() {
        chains = grokplan::buildChains(act.data(), nAct, T.hostWords + HW_CAND, T.hostWords + HW_CNT, used, order1);
        if (K.trace) traceChains();
        if (grokplan::longestChain(chains) || aheadLaunched) {
            if (!nSecond && !aheadLaunched) wonSoFar(st, maxCand, nAct, 0u);
            int rc = fork();
            if (rc != LC_OK) return rc;
            grokplan::forEachQueued(chains, order1, [&](const grokplan::Step& s) { runStep(s, rc); });
            rc = join(rc);  // (always: a failure inside the forked region must not leave the worker streams unjoined)
            if (rc != LC_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
        return LC_OK;
    }

    // ---- the finish: the first contributing entry per value; its rows go out.  All of it returns at once when values are still in
    // play somewhere (gate != 0): the host then finishes those entries and queues it again.
    // What is left of phase 2 needs the survivors of the remainder screens -- almost always none.  Round 5: the host no longer waits
    // to learn that.  The screens add their survivors to the gate word, the finish of the batch is queued behind them (it returns at
    // once if the gate is up), and the host reads everything in ONE round trip: gate down = done (three host synchronisations per batch
    // instead of four); gate up = the search rounds of the entries with survivors, then the finish again.
    int finish(const uint32_t* g) {
        if (nAct) {
            hipLaunchKernelGGL(grok_entry_finish_kernel, dim3(grid(maxCand), nAct), dim3(kGrokPlanBlock), 0, st, T.dEntries, winner, undecided, g, 0u);
        }
        hipLaunchKernelGGL(grok_resolve_kernel, dim3(grid(n)), dim3(kGrokPlanBlock), 0, st, n, winner, undecided, d_pattern, g);
        if (nAct) {
            // (row nAct of the grid: the extra rows of the winners)
            hipLaunchKernelGGL(grok_commit_kernel, dim3(std::max(grid(maxCand), 64u), nAct + 1), dim3(kGrokPlanBlock), 0, st, T.dEntries, nAct, d_pattern,
                               d_first, row, g, xtmp, xcount, xcap, xstride, map, d_extra, extraCap, d_nextra, T.dTail + TW_NEXTRA);
        }
        HIP_TRY(hipGetLastError());
        // (tail words, the copy of nextra among them, and the entries' counters: one block)
        HIP_TRY(hipMemcpyAsync(T.hostWords + HW_TAIL, T.dTail, (64 + size_t(nAct) * GC_WORDS) * 4, hipMemcpyDeviceToHost, st));
        if (tlsTail.armed) {
            HIP_TRY(hipMemcpyAsync(tlsTail.hPattern, d_pattern, size_t(n) * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(tlsTail.hFirst, d_first, size_t(n) * row * 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(syncCounted(st));  // sync 3 = the last one, unless the gate is up
        if (tlsTail.armed) {
            tlsTail.done = true;
            tlsTail.nextra = T.hostWords[HW_TAIL + TW_NEXTRA];
        }
        return LC_OK;
    }

    // ---- behind the finish: what the chains measured, and the search rounds of the entries with survivors
    void afterCounts() {
        if (calibrate)
            for (size_t a = 0; a < nAct; ++a)
                if (act[a].busy) learn(patterns[act[a].p].re->grokCost1Ns, T.tick[2 * nAct + 2 * a], T.tick[2 * nAct + 2 * a + 1], act[a].cand);
        // (the entries' histories: do most of the slots in play pass the remainder screen?  Judged on the batches that ran the screen
        // for the entry -- every calibration batch does)
        for (size_t a = 0; a < nAct; ++a) {
            const bool early = (chains.earlyMask >> a) & 1ull;
            if (K.trace && cnt(a, GC_ROUND0))
                fprintf(stderr, "grok plan 2d: entry %u in play %u, remainder passes the screen %u%s\n", act[a].p, cnt(a, GC_ROUND0),
                        cnt(a, GC_REMAINDER), early ? " (rounds queued ahead)" : "");
            const int seen = early ? -1 : grokplan::nextRemainderSeen(cnt(a, GC_ROUND0), cnt(a, GC_REMAINDER));
            if (seen >= 0) patterns[act[a].p].re->grokRemainderSeen.store(uint32_t(seen), std::memory_order_relaxed);
        }
    }
    int survivors() {
        afterCounts();
        if (T.hostWords[HW_TAIL + TW_GATE] == 0) return LC_OK;
        // (the survivors' share leaves the gate again: what stays up is what the queued rounds left in play)
        hipLaunchKernelGGL(grok_survivor_gate_kernel, dim3(1), dim3(64), 0, st, static_cast<const GrokEntryDev*>(T.dEntries), nAct, gate, 0u);
        bool any = false;
        for (size_t a = 0; a < nAct; ++a) any = any || (cnt(a, GC_REMAINDER) && !act[a].queued);
        if (!any) return LC_OK;
        std::vector<size_t> byCost;  // (dearest first, by the static estimate)
        for (size_t a = 0; a < nAct; ++a) byCost.push_back(a);
        std::sort(byCost.begin(), byCost.end(), [&](size_t x, size_t y) { return act[x].cost > act[y].cost; });
        int rc = fork();
        if (rc != LC_OK) return rc;
        std::vector<grokplan::Step> steps;
        for (size_t i = 0; i < nAct && rc == LC_OK; ++i) {
            const size_t a = byCost[i];
            PlanEntry& e = act[a];
            if (!cnt(a, GC_REMAINDER) || e.queued) continue;
            if (K.trace) fprintf(stderr, "grok plan 2e: entry %u in play %u survivors %u\n", e.p, cnt(a, GC_ROUND0), cnt(a, GC_REMAINDER));
            steps.clear();
            grokplan::appendRounds(e, a, true, steps);
            for (const grokplan::Step& s : steps) runStep(s, rc);
        }
        rc = join(rc);
        return rc != LC_OK ? rc : finish(gate);
    }

    // ---- values still in play after the last queued round of some entries: those entries go on, a stretch of rounds at a time (as
    // many again as they had queued, the counts on the device as before), until nothing is left -- an entry pays this once, then
    // asks for that many rounds ahead
    int deferred() {
        tPhase3 = msNow();
        if (T.hostWords[HW_TAIL + TW_GATE] == 0) return LC_OK;
        for (size_t a = 0; a < nAct; ++a) {
            PlanEntry& e = act[a];
            uint32_t* hostRounds = T.hostWords + HW_CNT + a * GC_WORDS + GC_ROUND0;
            uint32_t inPlay = hostRounds[e.rounds - 1];
            if (!inPlay) continue;
            ++stats.deferredEntries;
            const GrokDevicePattern& gp = patterns[e.p];
            uint32_t r = e.rounds;  // rounds done so far
            while (inPlay) {
                const uint32_t stretch = std::min(kGrokMaxRounds, std::max(4u, r));
                // the list of round r was written by round r - 1: (r & 1) ? listA : listB; counters are reused from slot 0
                HIP_TRY(hipMemsetAsync(e.dev.cnt + GC_ROUND0, 0, size_t(stretch) * 4, st));
                for (uint32_t k = 0; k < stretch; ++k, ++r) {
                    const uint32_t* list = (r & 1) ? e.dev.listA : e.listB;
                    uint32_t* out = (r & 1) ? e.listB : e.dev.listA;
                    const uint32_t bound = k == 0 ? inPlay : e.cand;
                    const uint32_t* countPtr = k == 0 ? nullptr : e.dev.cnt + GC_ROUND0 + k - 1;
                    if (const int rc = lcMatchOnStream(gp.re, gp.re->engine, entryBatch(e, bound, countPtr, list, e.dev.from, st)); rc != LC_OK) return rc;
                    hipLaunchKernelGGL(grok_advance2_kernel, dim3(grid(bound)), dim3(kGrokPlanBlock), 0, st, list, bound, countPtr, e.status, e.caps,
                                       e.capsRow, e.columns, e.dev, xtmp, xcap, xstride, xcount, out, e.dev.cnt + GC_ROUND0 + k,
                                       static_cast<uint32_t*>(nullptr));
                }
                HIP_TRY(hipMemcpyAsync(hostRounds, e.dev.cnt + GC_ROUND0, size_t(stretch) * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(syncCounted(st));
                inPlay = hostRounds[stretch - 1];
                if (!inPlay) {  // rounds that had anything to search: up to the first empty list of this stretch
                    uint32_t usedRounds = stretch;
                    while (usedRounds > 1 && hostRounds[usedRounds - 2] == 0) --usedRounds;
                    r = r - stretch + usedRounds;
                }
            }
            e.ran = r;  // (what this batch needed: the hint below)
        }
        return finish(nullptr);
    }

    // ---- the entries' histories: wide first next time?  how many rounds to queue ahead?  (grok_plan_host.hpp has the rules)
    void history() {
        for (size_t a = 0; a < nAct; ++a) {
            const PlanEntry& e = act[a];
            const uint32_t* my = T.hostWords + HW_CNT + a * GC_WORDS;
            std::atomic<uint32_t>& overflowSeen = firstOf(e)->grokOverflowSeen;
            const uint32_t seen = overflowSeen.load(std::memory_order_relaxed);
            if (my[GC_WIDE] || seen) overflowSeen.store(grokplan::nextOverflowSeen(seen, my[GC_WIDE]), std::memory_order_relaxed);
            lc_regex* re = patterns[e.p].re;
            const grokplan::RoundsHint now{re->grokRounds.load(std::memory_order_relaxed), re->grokRoundsSlack.load(std::memory_order_relaxed)};
            const grokplan::RoundsHint next = grokplan::nextRoundsHint(now, e.ran, grokplan::roundsNeeded(my, e.rounds, e.ran));
            if (next.rounds != now.rounds) re->grokRounds.store(next.rounds, std::memory_order_relaxed);
            re->grokRoundsSlack.store(next.slack, std::memory_order_relaxed);
        }
    }

    int result() {
        if (K.trace)
            fprintf(stderr, "grok plan: n %u entries %u (second pass %u) pairs %u screens %u | phase1 %.3f ms, entries+finish %.3f ms, total %.3f ms, syncs %u, deferred %u\n",
                    n, nAct, nSecond, stats.pairs, P1.nScreens, tPhase1, tPhase3 - tPhase1, msNow(), stats.hostSyncs, stats.deferredEntries);
        const uint32_t xWanted = T.hostWords[HW_TAIL + TW_XCOUNT];
        const uint32_t nextra = T.hostWords[HW_TAIL + TW_NEXTRA];
        if (xWanted > xcap) {
            // the temporary rows themselves did not fit: report an upper bound of what is needed (winners' rows <= all rows)
            HIP_TRY(hipMemcpy(d_nextra, &xWanted, 4, hipMemcpyHostToDevice));
            lcSetLastError("grok: " + std::to_string(xWanted) + " extra match rows needed, buffer holds " + std::to_string(extraCap));
            return LC_ERR_OVERFLOW;
        }
        if (nextra > extraCap) {
            lcSetLastError("grok: " + std::to_string(nextra) + " extra match rows needed, buffer holds " + std::to_string(extraCap));
            return LC_ERR_OVERFLOW;
        }
        return LC_OK;
    }
};

int grokMatchSpeculative(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, const GrokOptions& opts, uint32_t row,
                         const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, int32_t* d_pattern,
                         int32_t* d_first, int32_t* d_extra, uint32_t extraCap, uint32_t* d_nextra, void* d_scratch, hipStream_t st,
                         int dev) {
    GrokBatch B{patterns, state, opts, row, d_data, d_off, d_len, n, d_pattern, d_first, d_extra, extraCap, d_nextra, d_scratch, st, dev};
    int rc = B.phase1();  // sync 1
    if (rc == LC_OK) rc = B.entries();
    if (rc == LC_OK && B.nAct) rc = B.round0();
    if (rc == LC_OK && B.nAct) rc = B.ahead();  // sync 2
    if (rc == LC_OK && B.nAct) rc = B.runChains();
    if (rc == LC_OK) rc = B.finish(B.gate);  // sync 3: the last one, unless the gate is up
    if (rc == LC_OK && B.nAct) rc = B.survivors();
    if (rc == LC_OK) rc = B.deferred();
    if (rc != LC_OK) return rc;
    B.history();
    return B.result();
}
}  // namespace

int lcGrokMatchDevice(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, const GrokOptions& opts, uint32_t row,
                      const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, int32_t* d_pattern,
                      int32_t* d_first, int32_t* d_extra, uint32_t extraCap, uint32_t* d_nextra, void* d_scratch, size_t scratchBytes,
                      void* streamPtr) {
    tlsStats = GrokBatchStats{};
    if (n == 0) return LC_OK;
    if (!state || !d_data || !d_off || !d_len || !d_pattern || !d_first || !d_nextra || !d_scratch || (extraCap && !d_extra))
        return LC_ERR_ARG;
    if (scratchBytes < lcGrokScratchBytes(n, row)) {
        lcSetLastError("grok: scratch buffer too small");
        return LC_ERR_ARG;
    }
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    {
        const int rcDev = lcDeviceEntryDevice(d_data, &dev);
        if (rcDev != LC_OK) return rcDev;
    }
    hipStream_t st = static_cast<hipStream_t>(streamPtr);
    static const int forced = [] {  // LC_GROK_SPECULATIVE=0/1 overrides the handle's option (A/B measurements)
        const char* e = getenv("LC_GROK_SPECULATIVE");
        return e ? (e[0] == '0' ? 0 : 1) : -1;
    }();
    const bool speculative = (forced < 0 ? opts.speculative : forced != 0) && patterns.size() <= 64;
    tlsStats.speculative = speculative;
    if (speculative)
        return grokMatchSpeculative(patterns, state, opts, row, d_data, d_off, d_len, n, d_pattern, d_first, d_extra, extraCap, d_nextra,
                                    d_scratch, st, dev);
    return grokMatchSequential(patterns, state, opts, row, d_data, d_off, d_len, n, d_pattern, d_first, d_extra, extraCap, d_nextra,
                               d_scratch, st, dev);
}

// include/lc_grok.h: lc_grok_plan_masks_device (introspection for tests) -- phase 1 of the plan path as the matcher runs it for a batch
// of this n, then the masks (and the count words) copied out
int lcGrokPlanMasksDevice(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, uint32_t row, const uint8_t* d_data,
                          const uint32_t* d_off, const uint32_t* d_len, uint32_t n, int stage, uint64_t* d_masks, uint32_t* d_counts,
                          void* d_scratch, size_t scratchBytes, void* streamPtr) {
    if (n == 0) return LC_OK;
    if (!state || !d_data || !d_off || !d_len || !d_masks || !d_scratch || (stage != 1 && stage != 2) || patterns.size() > 64) return LC_ERR_ARG;
    if (scratchBytes < lcGrokScratchBytes(n, row)) {
        lcSetLastError("grok: scratch buffer too small");
        return LC_ERR_ARG;
    }
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    {
        const int rcDev = lcDeviceEntryDevice(d_data, &dev);
        if (rcDev != LC_OK) return rcDev;
    }
    hipStream_t st = static_cast<hipStream_t>(streamPtr);
    PlanThread& T = tlsPlan;
    {
        int rc = T.ensure(dev, 0);
        if (rc != LC_OK) return rc;
    }
    GrokPhase1 P1;
    {
        int rc = grokPlanPhase1(patterns, state, T, row, d_data, d_off, d_len, n, nullptr, nullptr, d_scratch, st, dev, stage, &P1);
        if (rc != LC_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(d_masks, P1.masks, size_t(n) * 8, hipMemcpyDeviceToDevice, st));
    if (stage == 2 && d_counts) HIP_TRY(hipMemcpyAsync(d_counts, T.dPlanWords, size_t(kPlanWords) * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    return LC_OK;
}

// include/lc_grok.h: lc_grok_screen_blob -- the screen grok_screen_all_kernel walks for an entry and what the plan stages of it
const std::vector<uint32_t>* lcGrokPlanScreenBlob(const GrokDevicePattern& gp, uint32_t* ldsBytes) {
    const lc_regex* scr = planScreenOf(gp);
    if (!scr) return nullptr;
    if (ldsBytes) *ldsBytes = planScreenLdsBytes(scr);
    return &scr->screenBlob;
}

int lcGrokSampleDevice(const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, uint32_t maxValues, void* streamPtr,
                       std::vector<uint8_t>& data, std::vector<uint32_t>& off, std::vector<uint32_t>& len) {
    data.clear();
    off.clear();
    len.clear();
    const uint32_t take = std::min(n, maxValues);
    if (!take) return LC_OK;
    int dev = 0;
    {
        const int rcDev = lcDeviceEntryDevice(d_data, &dev);
        if (rcDev != LC_OK) return rcDev;
    }
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(streamPtr)));  // (what the caller queued before the call has produced the batch)
    std::vector<uint32_t> o(take), l(take);
    HIP_TRY(hipMemcpy(o.data(), d_off, size_t(take) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(l.data(), d_len, size_t(take) * 4, hipMemcpyDeviceToHost));
    // one copy of the byte range the values span (batches are packed: the range is the values themselves)
    uint64_t lo = ~uint64_t(0), hi = 0;
    for (uint32_t i = 0; i < take; ++i) {
        lo = std::min<uint64_t>(lo, o[i]);
        hi = std::max<uint64_t>(hi, uint64_t(o[i]) + l[i]);
    }
    if (hi <= lo || hi - lo > (uint64_t(64) << 20)) return LC_OK;  // (nothing, or values strewn over more than is worth a sample)
    std::vector<uint8_t> range(size_t(hi - lo));
    HIP_TRY(hipMemcpy(range.data(), d_data + lo, range.size(), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < take; ++i) {
        off.push_back(uint32_t(data.size()));
        len.push_back(l[i]);
        data.insert(data.end(), range.begin() + long(o[i] - lo), range.begin() + long(o[i] - lo + l[i]));
    }
    return LC_OK;
}

// What a thread that calls lcGrokMatchHost keeps between calls (ProcessLogs hands over group after group): a stream of its own
// (runner threads must not meet on the null stream), pinned staging for the way in and the way out, device buffers; grow-only.
namespace {
struct GrokDev {
    void* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    void release() {
        if (p && lcRuntimeUsable()) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t bytes) {
        if (p && cap >= bytes) return hipSuccess;
        release();
        const size_t want = bytes + (bytes >> 2) + 256;
        hipError_t e = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
};
struct GrokHostThread {
    int device = -1;
    hipStream_t stream = nullptr;
    GrokDev dIn, dPattern, dFirst, dExtra, dNextra, dScratch;  // device
    GrokDev hIn, hOut, hExtra;                                 // pinned host
    GrokHostThread() { hIn.pinned = hOut.pinned = hExtra.pinned = true; }
    ~GrokHostThread() { release(); }
    void release() {
        if (device >= 0 && lcRuntimeUsable()) {
            int cur = 0;
            const bool haveCur = hipGetDevice(&cur) == hipSuccess;
            if (hipSetDevice(device) == hipSuccess) {
                if (stream) {
                    (void)hipStreamSynchronize(stream);
                    (void)hipStreamDestroy(stream);
                }
                for (GrokDev* d : {&dIn, &dPattern, &dFirst, &dExtra, &dNextra, &dScratch, &hIn, &hOut, &hExtra}) d->release();
            }
            if (haveCur) (void)hipSetDevice(cur);
        }
        stream = nullptr;
        device = -1;
    }
    int ensure(int dev) {
        if (device == dev) return LC_OK;
        release();
        lcRegisterExitHook();
        device = dev;
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return LC_OK;
    }
};
thread_local GrokHostThread tlsGrokHost;
}  // namespace
void lcGrokThreadRelease() {
    tlsGrokHost.release();
    tlsPlan.release();
}

// One group of one runner thread, as handed to lcGrokMatchHost.
struct GrokDeviceState::HostJob {
    const uint8_t* data;
    const uint32_t* off;
    const uint32_t* len;
    uint32_t n;
    int32_t* pattern;
    std::vector<int32_t>* first;      // the group's own rows (filled by its thread from firstSrc)
    std::vector<int32_t>* extraRows;  // [line, seq, row...] sorted, lines relative to the group
    const std::vector<GrokDevicePattern>* patterns;  // the call's view of the processor (anchored forms appear as the warm-up goes on)
    const GrokOptions* opts;
    uint32_t row;
    size_t bytes = 0;                 // sum of the group's value lengths (taken by its own thread before it queues)
    // where the group's values go in the batch's pinned staging (the worker's `place`), filled by the group's own thread (`gather`)
    uint8_t* hData = nullptr;
    uint32_t* hOff = nullptr;
    uint32_t* hLen = nullptr;
    uint32_t byteBase = 0;
    // results in the batch's pinned staging (the worker's `run`), taken out by the group's own thread
    const int32_t* patternSrc = nullptr;
    const int32_t* firstSrc = nullptr;
    const std::string* error = nullptr;  // the batch's message in the worker's batch state (the worker's last error is thread-local to the worker) ...
    std::string errorText;            // ... copied here by the job's own thread while the batch's state is still the batch's
    const GrokBatchStats* stats = nullptr;  // what the batch did (lc_grok_last_batch_stats is per calling thread)
    const std::string* kernels = nullptr;   // ... and which kernels it launched (lc_launched_kernels is per calling thread)
    uint32_t lines() const { return n; }
};

namespace {
// what the worker thread of one (processor, device) keeps between `place` and `run` of a batch
struct HostBatch {
    uint32_t n = 0;
    size_t bytes = 0, offAt = 0, lenAt = 0, inBytes = 0;
    std::string error, kernels;
    GrokBatchStats stats;
};
}  // namespace

struct GrokDeviceState::HostCombiner {
    GrokDeviceState* state = nullptr;
    int device = 0;
    HostBatch batch;
    std::unique_ptr<lccombine::GroupCombiner<HostJob>> combiner;
};

namespace {
using HostJob = GrokDeviceState::HostJob;

// `place`: the batch is fixed -- the values of all groups packed back to back (they may come from anywhere), then offsets and lengths:
// one pinned block, one copy.  Runs on the worker thread; every group's own thread then copies its values in (grokGatherJob).
int grokPlaceHostBatch(GrokDeviceState::HostCombiner& C, std::vector<HostJob*>& jobs) {
    HostBatch& B = C.batch;
    B = HostBatch{};
    GrokHostThread& H = tlsGrokHost;
    auto fail = [&](int rc) {
        B.error = lc_last_error();
        for (HostJob* j : jobs) j->error = &B.error;
        return rc;
    };
    {
        const int rc = H.ensure(C.device);
        if (rc != LC_OK) return fail(rc);
    }
    size_t n64 = 0;
    for (const HostJob* j : jobs) {
        B.bytes += j->bytes;
        n64 += j->n;
    }
    if (B.bytes > 0xFFFFFFF0ull || n64 > 0x7FFFFFFFull) {
        lcSetLastError("grok: more than 4 GiB of values in one batch");
        return fail(LC_ERR_ARG);
    }
    B.n = uint32_t(n64);
    B.offAt = alignUp(B.bytes + 16, 256);
    B.lenAt = B.offAt + alignUp(size_t(B.n) * 4, 256);
    B.inBytes = B.lenAt + size_t(B.n) * 4;
    if (H.hIn.ensure(B.inBytes) != hipSuccess || H.dIn.ensure(B.inBytes) != hipSuccess) {
        lcSetLastError("grok: staging allocation failed");
        return fail(LC_ERR_HIP);
    }
    uint8_t* hIn = static_cast<uint8_t*>(H.hIn.p);
    size_t at = 0;
    uint32_t k = 0;
    for (HostJob* j : jobs) {
        j->hData = hIn + at;
        j->byteBase = uint32_t(at);
        j->hOff = reinterpret_cast<uint32_t*>(hIn + B.offAt) + k;
        j->hLen = reinterpret_cast<uint32_t*>(hIn + B.lenAt) + k;
        at += j->bytes;
        k += j->n;
    }
    std::memset(hIn + at, 0, 16);
    return LC_OK;
}

// `gather`: on the group's OWN thread, all groups of a batch side by side
void grokGatherJob(HostJob& j) {
    uint32_t at = 0;
    for (uint32_t i = 0; i < j.n; ++i) {
        j.hOff[i] = j.byteBase + at;
        j.hLen[i] = j.len[i];
        std::memcpy(j.hData + at, j.data + j.off[i], j.len[i]);
        at += j.len[i];
    }
}

// `run`: the merged batch on the worker thread's stream; sets patternSrc / firstSrc / extraRows of every job
int grokRunHostBatch(GrokDeviceState::HostCombiner& C, std::vector<HostJob*>& jobs) {
    static const bool traceHost = getenv("LC_GROK_TRACE") != nullptr;
    const auto th0 = std::chrono::steady_clock::now();
    auto hostMs = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count(); };
    HostBatch& B = C.batch;
    GrokHostThread& H = tlsGrokHost;
    const std::vector<GrokDevicePattern>& patterns = *jobs.front()->patterns;
    const GrokOptions& opts = *jobs.front()->opts;
    const uint32_t row = jobs.front()->row, n = B.n;
    const size_t offAt = B.offAt, lenAt = B.lenAt, inBytes = B.inBytes;
    int rcAll = LC_OK;
    (void)lc_launched_kernels(nullptr, 0);  // (the worker's log: what THIS batch launches goes to the callers' logs)
    auto body = [&]() -> int {
    const size_t scratch = lcGrokScratchBytes(n, row);
    uint32_t extraCap = n / 4 + 1024;
    const size_t firstBytes = size_t(n) * row * 4;
    HIP_TRY(H.dPattern.ensure(size_t(n) * 4));
    HIP_TRY(H.dFirst.ensure(firstBytes));
    HIP_TRY(H.dNextra.ensure(4));
    HIP_TRY(H.dScratch.ensure(scratch));
    HIP_TRY(H.hOut.ensure(alignUp(size_t(n) * 4, 256) + firstBytes));
    int32_t* hPattern = static_cast<int32_t*>(H.hOut.p);
    int32_t* hFirst = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(H.hOut.p) + alignUp(size_t(n) * 4, 256));
    const uint8_t* dIn = static_cast<const uint8_t*>(H.dIn.p);
    HIP_TRY(hipMemcpyAsync(H.dIn.p, H.hIn.p, inBytes, hipMemcpyHostToDevice, H.stream));
    const double tGather = hostMs();
    uint32_t nExtra = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIP_TRY(H.dExtra.ensure(size_t(extraCap) * (row + 2) * 4));
        // (the speculative path queues the copies of the pattern ids and the first rows behind its last kernels: its second sync
        // covers them)
        tlsTail = GrokTailCopy{hPattern, hFirst, true, false};
        int rc = lcGrokMatchDevice(patterns, C.state, opts, row, dIn, reinterpret_cast<const uint32_t*>(dIn + offAt),
                                   reinterpret_cast<const uint32_t*>(dIn + lenAt), n, static_cast<int32_t*>(H.dPattern.p),
                                   static_cast<int32_t*>(H.dFirst.p), static_cast<int32_t*>(H.dExtra.p), extraCap,
                                   static_cast<uint32_t*>(H.dNextra.p), H.dScratch.p, scratch, H.stream);
        const bool copied = tlsTail.done;
        nExtra = tlsTail.nextra;
        tlsTail = GrokTailCopy{};
        if (rc == LC_ERR_OVERFLOW || !copied) {
            HIP_TRY(hipMemcpyAsync(hFirst, H.dNextra.p, 4, hipMemcpyDeviceToHost, H.stream));
            HIP_TRY(syncCounted(H.stream));
            nExtra = uint32_t(hFirst[0]);
        }
        if (rc == LC_ERR_OVERFLOW && attempt == 0) {
            extraCap = nExtra;  // the number needed is known now
            continue;
        }
        if (rc != LC_OK) return rc;
        if (!copied) {
            HIP_TRY(hipMemcpyAsync(hPattern, H.dPattern.p, size_t(n) * 4, hipMemcpyDeviceToHost, H.stream));
            HIP_TRY(hipMemcpyAsync(hFirst, H.dFirst.p, firstBytes, hipMemcpyDeviceToHost, H.stream));
            HIP_TRY(syncCounted(H.stream));
        }
        break;
    }
    const double tMatch = hostMs();
    const size_t w = row + 2;
    std::vector<uint32_t> idx(nExtra);
    const int32_t* raw = nullptr;
    if (nExtra) {
        HIP_TRY(H.hExtra.ensure(size_t(nExtra) * w * 4));
        HIP_TRY(hipMemcpyAsync(H.hExtra.p, H.dExtra.p, size_t(nExtra) * w * 4, hipMemcpyDeviceToHost, H.stream));
        HIP_TRY(syncCounted(H.stream));
        raw = static_cast<const int32_t*>(H.hExtra.p);
        // rows arrive in atomic order: sort by (line, seq)
        for (uint32_t i = 0; i < nExtra; ++i) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
            if (raw[a * w] != raw[b * w]) return raw[a * w] < raw[b * w];
            return raw[a * w + 1] < raw[b * w + 1];
        });
    }
    uint32_t base = 0, x = 0;
    B.stats = tlsStats;
    {
        char names[1024];
        (void)lc_launched_kernels(names, sizeof names);
        B.kernels = names;
    }
    for (HostJob* j : jobs) {
        j->stats = &B.stats;
        j->kernels = &B.kernels;
        j->patternSrc = hPattern + base;
        j->firstSrc = hFirst + size_t(base) * row;
        j->extraRows->clear();
        while (x < nExtra && uint32_t(raw[idx[x] * w]) < base + j->n) {
            const size_t at = j->extraRows->size();
            j->extraRows->resize(at + w);
            std::memcpy(j->extraRows->data() + at, &raw[idx[x] * w], w * 4);
            (*j->extraRows)[at] -= int32_t(base);
            ++x;
        }
        base += j->n;
    }
    if (traceHost)
        fprintf(stderr, "grok host batch: %zu groups %u values %zu bytes | H2D queued %.3f ms, device match %.3f ms, extra rows + hand-out %.3f ms\n",
                jobs.size(), n, B.bytes, tGather, tMatch - tGather, hostMs() - tMatch);
    return LC_OK;
    };
    rcAll = body();
    if (rcAll != LC_OK) {
        B.error = lc_last_error();
        for (HostJob* j : jobs) j->error = &B.error;
        (void)hipStreamSynchronize(H.stream);  // (nothing of a failed batch may still write the staging the next one reuses)
    }
    return rcAll;
}

GrokDeviceState::HostCombiner* grokCombinerFor(GrokDeviceState* state, int dev) {
    std::lock_guard<std::mutex> g(state->m);
    if (state->combiner[dev]) return state->combiner[dev];
    auto* C = new GrokDeviceState::HostCombiner();
    C->state = state;
    C->device = dev;
    lccombine::GroupCombiner<HostJob>::Hooks hooks;
    hooks.threadStart = [dev] { (void)lc_runtime_set_thread_device(dev); };  // the worker runs on the device of the threads it serves
    hooks.threadEnd = [] {
        if (lcRuntimeUsable()) lc_thread_release();  // the worker's plan, streams, pools and staging
    };
    hooks.place = [C](std::vector<HostJob*>& jobs) { return grokPlaceHostBatch(*C, jobs); };
    hooks.gather = [](HostJob& j) { grokGatherJob(j); };
    hooks.run = [C](std::vector<HostJob*>& jobs) { return grokRunHostBatch(*C, jobs); };
    lccombine::CombinerOptions o;
    if (const char* e = getenv("LC_GROK_LINGER_US")) o.lingerUs = unsigned(atoi(e));   // (A/B measurements)
    if (const char* e = getenv("LC_GROK_GAP_US")) o.gapUs = unsigned(atoi(e));
    C->combiner.reset(new lccombine::GroupCombiner<HostJob>(std::move(hooks), o));
    state->combiner[dev] = C;
    return C;
}
}  // namespace

static void grokFreeCombiners(GrokDeviceState* s) {
    for (int d = 0; d < kLcMaxDevices; ++d) {
        GrokDeviceState::HostCombiner* C = nullptr;
        {
            std::lock_guard<std::mutex> g(s->m);
            std::swap(C, s->combiner[d]);
        }
        if (!C) continue;
        C->combiner->stop();  // (groups still inside are answered first; the worker then releases what it holds on the device)
        delete C;
    }
}

int lcGrokCombinerStats(GrokDeviceState* state, uint64_t out[11]) {
    for (int i = 0; i < 11; ++i) out[i] = 0;
    if (!state) return LC_ERR_ARG;
    for (int d = 0; d < kLcMaxDevices; ++d) {
        GrokDeviceState::HostCombiner* C = nullptr;
        {
            std::lock_guard<std::mutex> g(state->m);
            C = state->combiner[d];
        }
        if (!C) continue;
        const lccombine::CombinerStats st = C->combiner->stats();
        out[0] += st.batches;
        out[1] += st.jobs;
        out[2] += st.lines;
        out[3] = std::max<uint64_t>(out[3], st.largestBatchJobs);
        out[4] += st.lingerExpired;
        out[5] += st.usIdle;
        out[6] += st.usLinger;
        out[7] += st.usPlace;
        out[8] += st.usGather;
        out[9] += st.usRun;
        out[10] += st.usTakeOut;
    }
    return LC_OK;
}

int lcGrokMatchHost(const std::vector<GrokDevicePattern>& patterns, GrokDeviceState* state, const GrokOptions& opts, uint32_t row,
                    const uint8_t* data, const uint32_t* off, const uint32_t* len, uint32_t n, int32_t* pattern,
                    const int32_t** firstRows, std::vector<int32_t>& extraRows) {
    *firstRows = nullptr;
    extraRows.clear();
    if (n == 0) return LC_OK;
    if (!state) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device");
        return LC_ERR_NO_DEVICE;
    }
    // Group commit (group_combiner.hpp).  ProcessorRunner hands over ONE ~1000-log group per call, from several threads that share the
    // plugin instance (core/runner/ProcessorRunner.cpp:138-142), and a batch costs the device about the same from 1 000 to 16 000 values
    // (it waits for its longest value, not for the chip).  The groups of the threads that call in together travel as ONE batch, run by
    // the worker thread of (this processor, the calling thread's device); the caller copies its own values in and its own rows out.
    int dev = 0;
    {
        const int rcDev = lcHostEntryDevice(&dev);  // the calling thread's binding decides the device
        if (rcDev != LC_OK) return rcDev;
    }
    thread_local std::vector<int32_t> tlsFirst;
    HostJob job{data, off, len, n, pattern, &tlsFirst, &extraRows, &patterns, &opts, row};
    for (uint32_t i = 0; i < n; ++i) job.bytes += len[i];
    GrokDeviceState::HostCombiner* C = grokCombinerFor(state, dev);
    const int rc = C->combiner->submit(job, [row](HostJob& j, int rcBatch) {
        if (rcBatch != LC_OK) {
            if (j.error) j.errorText = *j.error;
            return;
        }
        std::memcpy(j.pattern, j.patternSrc, size_t(j.n) * 4);
        j.first->resize(size_t(j.n) * row);
        std::memcpy(j.first->data(), j.firstSrc, size_t(j.n) * row * 4);
        if (j.stats) tlsStats = *j.stats;
        if (j.kernels) {
            size_t at = 0;
            while (at < j.kernels->size()) {
                size_t end = j.kernels->find(", ", at);
                if (end == std::string::npos) end = j.kernels->size();
                lcNoteKernel(j.kernels->substr(at, end - at).c_str());
                at = end + 2;
            }
        }
    });
    if (rc != LC_OK) {
        if (rc < 0) {
            lcSetLastError(rc == -1 ? "grok: the processor is shutting down" : "grok: the batch failed on the host (out of memory?)");
            return LC_ERR_ARG;
        }
        if (!job.errorText.empty()) lcSetLastError(job.errorText);
        return rc;
    }
    *firstRows = tlsFirst.data();
    return LC_OK;
}
