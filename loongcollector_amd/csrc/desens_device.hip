// desens_device.hip -- the engine level of processor_desensitize_gpu (include/lc_desensitize.h): the handle (compiled search, parsed
// rewrite), the round loop over the match entry of gpu_runtime.hip and the kernels of desens_kernel.hpp, and the host entry's trip
// through a runner thread's pinned staging.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lc_desensitize.h"
#include "desens_kernel.hpp"
#include "packed_trip.hpp"

using lcdesens::Batch;
using lcdesens::kBlock;
using lcdesens::Program;

namespace {
constexpr int kMaxDevices = 64;
constexpr uint64_t kMaxOutputBytes = 0xFFFFFFFFull;
}  // namespace

struct lc_desens {
    int method = LC_DESENS_CONST;
    bool replacingAll = false;
    lc_regex_t* re = nullptr;
    lcdesens::ParsedRewrite rewrite;
    uint32_t nGroups = 2;  // what every match call reports per value
    // the program as the kernels read it: [pieces | refGroup | literal bytes], uploaded once per device
    std::mutex uploadMutex;
    void* dProgram[kMaxDevices] = {};
    std::vector<uint8_t> blob;
    size_t refAt = 0, litAt = 0;
};

namespace {
// What RE2 refuses although the engines here can run it: look-arounds, atomic groups and possessive quantifiers.  The reference's Init
// fails on them, so the create call does (the rest of the dialect is the compiler's: LC_SYNTAX_REGEXP2).  nullptr: nothing found.
const char* refusedByRe2(const std::string& p) {
    for (size_t i = 0; i < p.size(); ++i) {
        const char c = p[i];
        if (c == '\\') {
            ++i;
        } else if (c == '[') {  // a class: to its closing bracket (a ']' right behind '[' or '[^' is a member)
            size_t j = i + 1;
            if (j < p.size() && p[j] == '^') ++j;
            if (j < p.size() && p[j] == ']') ++j;
            while (j < p.size() && p[j] != ']') j += p[j] == '\\' ? 2 : 1;
            i = j;
        } else if (c == '(' && i + 2 < p.size() && p[i + 1] == '?') {
            const char d = p[i + 2], e = i + 3 < p.size() ? p[i + 3] : 0;
            if (d == '=' || d == '!' || (d == '<' && (e == '=' || e == '!'))) return "invalid perl operator: a look-around";
            if (d == '>') return "invalid perl operator: an atomic group";
        } else if ((c == '*' || c == '+' || c == '?' || c == '}') && i + 1 < p.size() && p[i + 1] == '+') {
            bool quantifier = c != '}';
            if (!quantifier) {  // "{2}", "{2,}", "{2,3}" -- any other '}' is a literal
                size_t j = i;
                while (j > 0 && ((p[j - 1] >= '0' && p[j - 1] <= '9') || p[j - 1] == ',')) --j;
                quantifier = j > 0 && j < i && p[j - 1] == '{' && p[j] != ',';
            }
            if (quantifier) return "bad repetition operator: a possessive quantifier";
        }
    }
    return nullptr;
}
}  // namespace

extern "C" int lc_desens_create(int method, const char* before, size_t before_len, const char* content, size_t content_len, const char* replacing,
                                size_t replacing_len, int replacing_all, lc_desens_t** out, int* warning, char* err, size_t errcap) {
    if (warning) *warning = 0;
    if (err && errcap) err[0] = 0;
    if (!out || (method != LC_DESENS_CONST && method != LC_DESENS_MD5) || !before || !content || (method == LC_DESENS_CONST && !replacing && replacing_len))
        return LC_ERR_ARG;
    *out = nullptr;
    const std::string pattern = "(" + std::string(before, before_len) + ")" + std::string(content, content_len);
    if (const char* why = refusedByRe2(pattern)) {
        if (err && errcap) std::snprintf(err, errcap, "%s", why);
        return LC_ERR_SYNTAX;
    }
    lc_regex_t* re = nullptr;
    const int rc = lc_regex_compile(pattern.data(), pattern.size(), LC_SYNTAX_SEARCH | LC_SYNTAX_NO_DOTALL | LC_SYNTAX_NO_MULTILINE | LC_SYNTAX_REGEXP2,
                                    LC_ENGINE_AUTO, &re, err, errcap);
    if (rc != LC_OK) return rc;
    auto h = new lc_desens;
    h->method = method;
    h->replacingAll = replacing_all != 0;
    h->re = re;
    const int markCount = lc_regex_mark_count(re);  // the whole match, the `before` group, the user's groups
    if (method == LC_DESENS_CONST) {
        h->rewrite = lcdesens::parseRewrite("\\1" + std::string(replacing ? replacing : "", replacing_len), markCount - 1);
        if (h->rewrite.passThrough && warning) *warning = 1;
    }
    h->nGroups = h->rewrite.maxEngineGroup;
    const size_t pieceBytes = h->rewrite.pieces.size() * 4;
    h->refAt = pieceBytes;
    h->litAt = h->refAt + h->rewrite.refGroup.size() * 4;
    h->blob.assign(h->litAt + h->rewrite.lit.size() + 16, 0);
    if (pieceBytes) std::memcpy(h->blob.data(), h->rewrite.pieces.data(), pieceBytes);
    if (h->litAt > h->refAt) std::memcpy(h->blob.data() + h->refAt, h->rewrite.refGroup.data(), h->litAt - h->refAt);
    if (!h->rewrite.lit.empty()) std::memcpy(h->blob.data() + h->litAt, h->rewrite.lit.data(), h->rewrite.lit.size());
    *out = h;
    return LC_OK;
}

extern "C" void lc_desens_free(lc_desens_t* h) {
    if (!h) return;
    if (lcRuntimeUsable())
        for (void* p : h->dProgram)
            if (p) (void)hipFree(p);
    lc_regex_free(h->re);
    delete h;
}

extern "C" lc_regex_t* lc_desens_regex(const lc_desens_t* h) { return h ? h->re : nullptr; }

namespace {
// the handle's program on `dev`
int programOn(lc_desens* h, int dev, Program* P, const uint32_t** refGroup) {
    if (dev < 0 || dev >= kMaxDevices) return LC_ERR_ARG;
    std::lock_guard<std::mutex> lock(h->uploadMutex);
    if (!h->dProgram[dev]) {
        void* p = nullptr;
        LC_HIP_TRY(hipMalloc(&p, h->blob.size()));
        const hipError_t e = hipMemcpy(p, h->blob.data(), h->blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return lcHipFail(e, "hipMemcpy(desensitize program)");
        }
        h->dProgram[dev] = p;
    }
    const uint8_t* base = static_cast<const uint8_t*>(h->dProgram[dev]);
    *P = lcdesens::programOf(uint32_t(h->method), h->rewrite);
    P->pieces = reinterpret_cast<const uint32_t*>(base);
    P->lit = base + h->litAt;
    *refGroup = reinterpret_cast<const uint32_t*>(base + h->refAt);
    return LC_OK;
}

// per runner thread: the round loop's scratch, and the host entry's stream and staging; grow-only
struct DesensThread : TripThread<DesensThread> {
    TripBuf hIn, hOut, dIn, dOut, dFlags, dOutOff;                       // the host entry's
    TripBuf dCaps, dStatus, dState, dLists, dCount, dTileSums, hWord;    // the round loop's
    void* dRecs = nullptr;                                               // the cut records: grown by copying, see ensureRecs
    size_t recCap = 0;                                                   // in words
    int scratchDevice = -1;
    DesensThread() : TripThread(true) { hIn.pinned = hOut.pinned = hWord.pinned = true; }
    ~DesensThread() {
        if (lcRuntimeUsable() && (stream || scratchDevice >= 0)) release();
    }
    void releaseScratch() {
        for (TripBuf* b : {&dCaps, &dStatus, &dState, &dLists, &dCount, &dTileSums, &hWord}) b->release();
        if (dRecs) (void)hipFree(dRecs);
        dRecs = nullptr;
        recCap = 0;
        scratchDevice = -1;
    }
    void release() {
        releaseWith({&hIn, &hOut, &dIn, &dOut, &dFlags, &dOutOff});
        releaseScratch();
    }
};
thread_local DesensThread tlsDesens;

// room for usedWords + moreWords record words; what is there is kept (copied on `st`, which the caller has drained by the time the old
// block is freed: the copy is awaited here)
int ensureRecs(DesensThread& T, size_t usedWords, size_t moreWords, hipStream_t st) {
    const size_t want = usedWords + moreWords;
    if (T.dRecs && T.recCap >= want) return LC_OK;
    const size_t cap = want + (want >> 1) + 1024;
    void* p = nullptr;
    LC_HIP_TRY(hipMalloc(&p, cap * 4));
    if (T.dRecs && usedWords) {
        hipError_t e = hipMemcpyAsync(p, T.dRecs, usedWords * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return lcHipFail(e, "hipMemcpyAsync(desensitize records)");
        }
    }
    if (T.dRecs) (void)hipFree(T.dRecs);
    T.dRecs = p;
    T.recCap = cap;
    return LC_OK;
}

inline uint32_t blocksFor(uint64_t items, uint32_t perBlock) { return uint32_t((items + perBlock - 1) / perBlock); }

// Where the output bytes go once their total is known: room(total) -> the device pointer, or nullptr with *rc set.
template <class Room>
int applyOnStream(lc_desens* h, int dev, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, uint8_t* d_flags,
                  uint64_t* d_out_off, Room room, uint64_t* needed, lc_desens_stats_t* stats, hipStream_t st) {
    DesensThread& T = tlsDesens;
    if (T.scratchDevice != dev) {
        if (T.scratchDevice >= 0) T.releaseScratch();
        T.scratchDevice = dev;
    }
    Program P;
    const uint32_t* dRefGroup = nullptr;
    if (const int rc = programOn(h, dev, &P, &dRefGroup); rc != LC_OK) return rc;
    const bool md5 = h->method == LC_DESENS_MD5;
    const uint32_t G = h->nGroups, W = lcdesens::recWords(P);
    // scratch: the engine's rows; the state arrays; two lists; two count words; the scan's tile sums
    const size_t nUp = tripRoundUp(size_t(n), 64);
    LC_HIP_TRY(T.dCaps.ensure(size_t(n) * 2 * G * 4));
    LC_HIP_TRY(T.dStatus.ensure(nUp));
    LC_HIP_TRY(T.dState.ensure(nUp * 4 * 6 + nUp));
    LC_HIP_TRY(T.dLists.ensure(nUp * 4 * 2));
    LC_HIP_TRY(T.dCount.ensure(64));
    LC_HIP_TRY(T.hWord.ensure(64));
    const uint32_t nTiles = blocksFor(uint64_t(n) + 1, lcdesens::kScanTile);
    LC_HIP_TRY(T.dTileSums.ensure(size_t(nTiles) * 8));
    uint32_t* state = static_cast<uint32_t*>(T.dState.p);
    Batch b{d_data, d_off, state, state + nUp, state + 2 * nUp, state + 3 * nUp, reinterpret_cast<uint8_t*>(state + 6 * nUp),
            state + 4 * nUp, state + 5 * nUp, n};
    uint32_t* lists[2] = {static_cast<uint32_t*>(T.dLists.p), static_cast<uint32_t*>(T.dLists.p) + nUp};
    uint32_t* dCount = static_cast<uint32_t*>(T.dCount.p);
    int32_t* dCaps = static_cast<int32_t*>(T.dCaps.p);
    uint8_t* dStatus = static_cast<uint8_t*>(T.dStatus.p);
    volatile uint32_t* hWord = static_cast<volatile uint32_t*>(T.hWord.p);

    hipLaunchKernelGGL(lcdesens::desens_init_kernel, dim3(blocksFor(n, kBlock)), dim3(kBlock), 0, st, b, d_len, md5, lists[0]);
    LC_HIP_TRY(hipGetLastError());
    uint32_t active = n, round = 0;
    size_t usedWords = 0;
    uint64_t searches = 0;
    while (active) {
        if (const int rc = ensureRecs(T, usedWords, size_t(active) * W, st); rc != LC_OK) return rc;
        // the search: round 0 over every value from its first byte; later rounds over the list -- `const` resumed inside the whole value,
        // `md5` afresh on the suffix the private offset / length copy names
        int rc;
        if (round > 0) lcNoteKernel("desens_search_again");  // (lc_launched_kernels folds names: this one says a call took a second match launch)
        if (round == 0) rc =lc_regex_match_device_from(h->re, LC_ENGINE_AUTO, d_data, d_off, b.len, 0, n, nullptr, nullptr, nullptr, G, dCaps, dStatus, st);
        else if (md5) rc = lc_regex_match_device_from(h->re, LC_ENGINE_AUTO, d_data, b.offP, b.lenP, 0, active, lists[round & 1], nullptr, nullptr, G, dCaps, dStatus, st);
        else rc = lc_regex_match_device_from(h->re, LC_ENGINE_AUTO, d_data, d_off, b.len, 0, active, lists[round & 1], nullptr, b.from, G, dCaps, dStatus, st);
        if (rc != LC_OK) return rc;
        searches += active;
        uint32_t* countOut = dCount + ((round + 1) & 1);
        LC_HIP_TRY(hipMemsetAsync(countOut, 0, 4, st));
        lcNoteKernel("desens_collect_kernel");
        hipLaunchKernelGGL(lcdesens::desens_collect_kernel, dim3(blocksFor(active, kBlock)), dim3(kBlock), 0, st, b, P, dRefGroup, h->replacingAll,
                           lists[round & 1], active, dCaps, 2 * G, dStatus, static_cast<uint32_t*>(T.dRecs), uint32_t(usedWords / W),
                           lists[(round + 1) & 1], countOut);
        LC_HIP_TRY(hipGetLastError());
        usedWords += size_t(active) * W;
        ++round;
        if (!h->replacingAll) break;  // one round, and nothing to read
        LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord), countOut, 4, hipMemcpyDeviceToHost, st));
        LC_HIP_TRY(hipStreamSynchronize(st));
        active = hWord[0];
        if (active > n) {
            lcSetLastError("lc_desens_apply: the device-side count of active values is out of range");
            return LC_ERR_HIP;
        }
        if (usedWords / W + active > 0xFFFFFFF0ull) {
            lcSetLastError("lc_desens_apply: more than 2^32 cuts in one trip");
            return LC_ERR_OVERFLOW;
        }
    }
    if (stats) {
        stats->rounds = round;
        stats->pass_through = 0;
        stats->searches = searches;
    }
    lcNoteKernel("desens_size_kernel");
    hipLaunchKernelGGL(lcdesens::desens_size_kernel, dim3(blocksFor(uint64_t(n) + 1, kBlock)), dim3(kBlock), 0, st, b, P,
                       static_cast<const uint32_t*>(T.dRecs), d_flags, d_out_off);
    uint64_t* tileSums = static_cast<uint64_t*>(T.dTileSums.p);
    hipLaunchKernelGGL(lcdesens::desens_scan_sums_kernel, dim3(nTiles), dim3(kBlock), 0, st, d_out_off, n + 1, tileSums);
    hipLaunchKernelGGL(lcdesens::desens_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, tileSums, nTiles);
    hipLaunchKernelGGL(lcdesens::desens_scan_apply_kernel, dim3(nTiles), dim3(kBlock), 0, st, d_out_off, n + 1, tileSums);
    LC_HIP_TRY(hipGetLastError());
    LC_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(hWord) + 2, d_out_off + n, 8, hipMemcpyDeviceToHost, st));
    LC_HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = uint64_t(hWord[2]) | uint64_t(hWord[3]) << 32;
    if (needed) *needed = total;
    if (total > kMaxOutputBytes) {
        lcSetLastError("lc_desens_apply: the trip's output would pass 2^32 - 1 bytes");
        return LC_ERR_OVERFLOW;
    }
    if (total == 0) return LC_OK;
    int rc = LC_OK;
    uint8_t* d_out = room(total, &rc);
    if (!d_out) return rc;
    lcNoteKernel("desens_write_kernel");
    hipLaunchKernelGGL(lcdesens::desens_write_kernel, dim3(blocksFor(n, lcdesens::kWavesPerBlock)), dim3(kBlock), 0, st, b, P,
                       static_cast<const uint32_t*>(T.dRecs), d_out_off, d_out);
    LC_HIP_TRY(hipGetLastError());
    // (the scratch the kernels read is the calling thread's: it must not be reused by the thread's next call before they are through)
    LC_HIP_TRY(hipStreamSynchronize(st));
    return LC_OK;
}

// a pass-through handle: every value unchanged, nothing launched but the fill
int passThrough(uint32_t n, uint8_t* d_flags, uint64_t* d_out_off, uint64_t* needed, lc_desens_stats_t* stats, hipStream_t st) {
    LC_HIP_TRY(hipMemsetAsync(d_flags, 0, n, st));
    LC_HIP_TRY(hipMemsetAsync(d_out_off, 0, (size_t(n) + 1) * 8, st));
    LC_HIP_TRY(hipStreamSynchronize(st));
    if (needed) *needed = 0;
    if (stats) *stats = lc_desens_stats_t{0, 1, 0};
    return LC_OK;
}
}  // namespace

void lcDesensThreadRelease() { tlsDesens.release(); }

extern "C" int lc_desens_apply_device(lc_desens_t* h, const uint8_t* d_data, const uint32_t* d_off, const uint32_t* d_len, uint32_t n, uint8_t* d_flags,
                                      uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, uint64_t* needed, lc_desens_stats_t* stats, void* stream) {
    if (needed) *needed = 0;
    if (stats) *stats = lc_desens_stats_t{0, 0, 0};
    if (!h) return LC_ERR_ARG;
    if (n == 0) {  // out_off has n + 1 entries
        if (d_out_off) LC_HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, static_cast<hipStream_t>(stream)));
        return LC_OK;
    }
    if (!d_data || !d_off || !d_flags || !d_out_off || (!d_out && out_cap) || (reinterpret_cast<uintptr_t>(d_out_off) & 7)) return LC_ERR_ARG;
    if (lc_device_count() <= 0) {
        lcSetLastError("no HIP device: the desensitize processor has no CPU path");
        return LC_ERR_NO_DEVICE;
    }
    int dev = 0;
    const int rcDev = lcDeviceEntryDevice(d_data, &dev);
    if (rcDev != LC_OK) return rcDev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    lcRegisterExitHook();
    if (h->rewrite.passThrough) return passThrough(n, d_flags, d_out_off, needed, stats, st);
    return applyOnStream(h, dev, d_data, d_off, d_len, n, d_flags, d_out_off,
                         [&](uint64_t total, int* rc) -> uint8_t* {
                             if (total <= out_cap) return d_out;
                             lcSetLastError("lc_desens_apply_device: the output needs " + std::to_string(total) + " bytes");
                             *rc = LC_ERR_OVERFLOW;
                             return nullptr;
                         },
                         needed, stats, st);
}

// ------------------------------------------------------------------------------------------------ host values
namespace {
constexpr size_t kChunkBytes = 32u << 20;   // payload bytes per trip
constexpr uint32_t kChunkLines = 1u << 18;  // and at most this many values
constexpr size_t kChunkResultBytes = 64u << 20;
constexpr size_t kLineResultBytes = 8 + 1;  // out_off, flags
}  // namespace

extern "C" int lc_desens_apply_host(lc_desens_t* h, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint64_t* out_off,
                                    uint8_t** out, lc_desens_stats_t* stats) {
    if (out) *out = nullptr;
    if (stats) *stats = lc_desens_stats_t{0, 0, 0};
    if (!h || !out || !out_off) return LC_ERR_ARG;
    out_off[0] = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !flags) return LC_ERR_ARG;
    if (h->rewrite.passThrough) {  // (defined_only: nothing to ask the device)
        std::memset(flags, 0, n);
        std::memset(out_off, 0, (size_t(n) + 1) * 8);
        if (stats) stats->pass_through = 1;
        return LC_OK;
    }
    DesensThread& T = tlsDesens;
    int dev = 0;
    const int rcBegin = lcTripBegin(T, &dev, "no HIP device: the desensitize processor has no CPU path");
    if (rcBegin != LC_OK) return rcBegin;
    std::vector<uint8_t> bytes;
    lc_desens_stats_t total{0, 0, 0};
    // the input half of the packed trip alone (packed_trip.hpp): the result sizes are known only once applyOnStream is through
    const PackedTripSpec spec{"lc_desens_apply_host", "value", kChunkLines, kChunkBytes, kLineResultBytes, kChunkResultBytes, nullptr};
    PackedChunk c;
    while (c.next < n) {
        if (const int rc = packedTripPlan(T, spec, len, n, &c); rc != LC_OK) return rc;
        const uint32_t next = c.next, cnt = c.cnt;
        LC_HIP_TRY(T.dFlags.ensure(tripRoundUp(cnt, 64)));
        LC_HIP_TRY(T.dOutOff.ensure((size_t(cnt) + 1) * 8));
        if (const int rc = packedTripUpload(T, lines, len, c); rc != LC_OK) return rc;
        uint8_t* dIn = c.dIn;
        const size_t offAt = c.in.offAt;
        uint64_t needed = 0;
        lc_desens_stats_t s{0, 0, 0};
        hipError_t roomError = hipSuccess;
        int rc = applyOnStream(h, dev, dIn, reinterpret_cast<const uint32_t*>(dIn + offAt), nullptr, cnt, static_cast<uint8_t*>(T.dFlags.p),
                               static_cast<uint64_t*>(T.dOutOff.p),
                               [&](uint64_t totalBytes, int* rcRoom) -> uint8_t* {
                                   roomError = T.dOut.ensure(size_t(totalBytes));
                                   if (roomError == hipSuccess) return static_cast<uint8_t*>(T.dOut.p);
                                   *rcRoom = lcHipFail(roomError, "T.dOut.ensure(output bytes)");
                                   return nullptr;
                               },
                               &needed, &s, T.stream);
        if (rc == LC_OK && bytes.size() + needed > kMaxOutputBytes) {
            lcSetLastError("lc_desens_apply_host: the call's output would pass 2^32 - 1 bytes");
            rc = LC_ERR_OVERFLOW;
        }
        // the results come down: out_off, flags, then the bytes -- one trip's end for all three
        const size_t flagsAt = (size_t(cnt) + 1) * 8;
        const size_t bytesAt = tripRoundUp(flagsAt + cnt, 64);
        if (rc == LC_OK) {
            const hipError_t e = T.hOut.ensure(bytesAt + size_t(needed));
            if (e != hipSuccess) rc = lcHipFail(e, "T.hOut.ensure(results)");
        }
        uint8_t* hOut = static_cast<uint8_t*>(T.hOut.p);
        if (rc == LC_OK) {
            hipError_t e = hipMemcpyAsync(hOut, T.dOutOff.p, flagsAt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hOut + flagsAt, T.dFlags.p, cnt, hipMemcpyDeviceToHost, T.stream);
            if (e == hipSuccess && needed) e = hipMemcpyAsync(hOut + bytesAt, T.dOut.p, size_t(needed), hipMemcpyDeviceToHost, T.stream);
            if (e != hipSuccess) rc = lcHipFail(e, "hipMemcpyAsync(desensitize results)");
        }
        rc = T.end(rc);
        if (rc != LC_OK) return rc;
        const uint64_t base = bytes.size();
        const uint64_t* chunkOff = reinterpret_cast<const uint64_t*>(hOut);
        for (uint32_t i = 0; i <= cnt; ++i) out_off[next + i] = base + chunkOff[i];
        std::memcpy(flags + next, hOut + flagsAt, cnt);
        bytes.insert(bytes.end(), hOut + bytesAt, hOut + bytesAt + needed);
        total.rounds += s.rounds;
        total.searches += s.searches;
        c.advance(len);
    }
    if (stats) *stats = total;
    if (!bytes.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(bytes.size()));
        if (!*out) return LC_ERR_ARG;
        std::memcpy(*out, bytes.data(), bytes.size());
    }
    return LC_OK;
}
