// tests/native/desens_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_desensitize_gpu on a box without a GPU.
//
// csrc/processor_desensitize_gpu.cpp (Init, the gather, the per-event rules, the one copy into the SourceBuffer, counters, alarms) asks
// the engine for lc_desens_create / lc_desens_apply_host / lc_desens_free.  This translation unit answers them on the CPU: every SEARCH
// is answered by the oracle's matcher (oracle/bt_regex.c, the flags the model uses), and everything behind the search is the PRODUCT's --
// collectStep, outLen, writeValue, md5Hex and parseRewrite of csrc/desens_vm.hpp, the functions the kernels run, compiled here for the
// host and walked value by value (walkValue), each value from an exactly-sized heap block.  tests/helpers/desensitize_product.py builds
// processor_desensitize_gpu.cpp + event_model.cpp + this file into tests/_build/libdesens_double.so.  Never linked into
// loongcollector_amd/lib.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lc_desensitize.h"
#include "../../loongcollector_amd/csrc/desens_vm.hpp"
#include "../../loongcollector_amd/csrc/event_model.hpp"
#include "../../oracle/bt_regex.h"

static int gFailNext = 0, gGiveUpEvery = 0;
static uint64_t gApplyCalls = 0;

struct lc_desens {
    int method = 0;
    bool replacingAll = false;
    orx_prog* rx = nullptr;
    lcdesens::ParsedRewrite rewrite;
    uint32_t nGroups = 2;
};

extern "C" {
int lc_device_count(void) { return 1; }
const char* lc_last_error(void) { return "the double was told to fail this trip"; }

int lc_desens_create(int method, const char* before, size_t before_len, const char* content, size_t content_len, const char* replacing,
                     size_t replacing_len, int replacing_all, lc_desens_t** out, int* warning, char* err, size_t errcap) {
    if (warning) *warning = 0;
    const std::string pattern = "(" + std::string(before, before_len) + ")" + std::string(content, content_len);
    orx_prog* rx = orx_compile(pattern.data(), pattern.size(), ORX_NO_MOD_S | ORX_NO_MOD_M | ORX_REGEXP2, err, errcap);
    if (!rx) return LC_ERR_SYNTAX;
    auto h = new lc_desens;
    h->method = method;
    h->replacingAll = replacing_all != 0;
    h->rx = rx;
    if (method == LC_DESENS_CONST) {
        h->rewrite = lcdesens::parseRewrite("\\1" + std::string(replacing ? replacing : "", replacing_len), orx_mark_count(rx));
        if (h->rewrite.passThrough && warning) *warning = 1;
    }
    h->nGroups = uint32_t(orx_mark_count(rx)) + 1;
    *out = h;
    return LC_OK;
}
void lc_desens_free(lc_desens_t* h) {
    if (!h) return;
    orx_free(h->rx);
    delete h;
}
lc_regex_t* lc_desens_regex(const lc_desens_t*) { return nullptr; }

// one value: -> flags; out receives the new bytes of a changed value
static uint8_t walkOne(lc_desens_t* h, const uint8_t* value, uint32_t n, bool giveUp, std::vector<uint8_t>& out, uint32_t* rounds) {
    // exactly-sized: a read behind the value is an out-of-bounds read of this heap block
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(copy.get(), value, n);
    const lcdesens::Program P = lcdesens::programOf(uint32_t(h->method), h->rewrite);
    uint8_t flags = 0;
    lcdesens::walkValue(
        P, h->rewrite, h->replacingAll, copy.get(), n, h->nGroups,
        [&](uint32_t from, bool fresh, int32_t* caps) -> uint8_t {
            if (giveUp) return 3;  // LC_GAVE_UP
            // the oracle's row: group 0 the whole match, group 1 the `before` group -- the engine's groups 1 and 2
            const uint8_t* text = copy.get();
            const int r = fresh ? orx_search(h->rx, text + from, n - from, 0, caps) : orx_search(h->rx, text, n, from, caps);
            return r < 0 ? 3 : r == 0 ? 0 : 1;
        },
        out, &flags, rounds);
    return flags;
}

int lc_desens_apply_host(lc_desens_t* h, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint64_t* out_off,
                         uint8_t** out, lc_desens_stats_t* stats) {
    if (out) *out = nullptr;
    if (stats) *stats = lc_desens_stats_t{0, 0, 0};
    if (!h || !out || !out_off || (n && (!lines || !len || !flags))) return LC_ERR_ARG;
    if (gFailNext) {
        --gFailNext;
        return LC_ERR_HIP;
    }
    ++gApplyCalls;
    out_off[0] = 0;
    std::vector<uint8_t> bytes, one;
    uint32_t rounds = 0;
    for (uint32_t i = 0; i < n; ++i) {
        one.clear();
        uint32_t r = 0;
        if (h->rewrite.passThrough) flags[i] = 0;
        else flags[i] = walkOne(h, lines[i], len[i], gGiveUpEvery && (i + 1) % uint32_t(gGiveUpEvery) == 0, one, &r);
        if (flags[i] & LC_DESENS_CHANGED) bytes.insert(bytes.end(), one.begin(), one.end());
        out_off[i + 1] = bytes.size();
        rounds = r > rounds ? r : rounds;
    }
    if (stats) {
        stats->rounds = rounds;
        stats->pass_through = h->rewrite.passThrough ? 1 : 0;
    }
    if (!bytes.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(bytes.size()));
        std::memcpy(*out, bytes.data(), bytes.size());
    }
    return LC_OK;
}

// MD5 of the product's routine, from an exactly-sized block
void dd_md5(const uint8_t* p, uint32_t len, uint8_t* out32) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(copy.get(), p, len);
    lcdesens::md5Hex(copy.get(), len, out32);
}
// the parsed rewrite as text: "L<hex>" per literal piece, "G<engine group>" per group piece, blank separated; "PASS" for the error path
char* dd_rewrite_text(const char* rewrite, size_t len, int re2Groups) {
    const lcdesens::ParsedRewrite R = lcdesens::parseRewrite(std::string(rewrite, len), re2Groups);
    std::string s;
    if (R.passThrough) s = "PASS";
    for (size_t k = 0; !R.passThrough && k < R.pieces.size() / 3; ++k) {
        if (!s.empty()) s += " ";
        if (R.pieces[3 * k] == lcdesens::kPieceLiteral) {
            s += "L";
            char hex[3];
            for (uint32_t q = 0; q < R.pieces[3 * k + 2]; ++q) {
                std::snprintf(hex, sizeof hex, "%02x", R.lit[R.pieces[3 * k + 1] + q]);
                s += hex;
            }
        } else {
            s += "G" + std::to_string(R.refGroup[R.pieces[3 * k + 1]]);
        }
    }
    return strdup(s.c_str());
}
// The per-value routine alone over values that lie back to back in ONE resident buffer (value i = data[off[i] .. off[i + 1])) and
// PRECOMPUTED cuts (cutCount[i] engine rows of 2 * G offsets each, in value order): the chains are built first, then outLen + writeValue
// run over every value into `out` (as large as the caller knows the output to be) -- what tools/desensitize_bench.py times as "the
// per-value routine on one host thread".  -> the bytes written; *seconds: the timed part
uint64_t dd_write_resident(lc_desens_t* h, const uint8_t* data, const uint32_t* off, uint32_t n, const uint32_t* cutCount, const int32_t* rows, uint32_t G,
                           uint8_t* out, double* seconds) {
    const lcdesens::Program P = lcdesens::programOf(uint32_t(h->method), h->rewrite);
    const uint32_t W = lcdesens::recWords(P);
    uint64_t nCuts = 0;
    for (uint32_t i = 0; i < n; ++i) nCuts += cutCount[i];
    std::vector<uint32_t> recs(size_t(nCuts ? nCuts : 1) * W), last(n);
    std::vector<int32_t> row(2 * size_t(G));
    uint32_t rec = 0;
    for (uint32_t i = 0; i < n; ++i) {
        lcdesens::ValueState S;
        uint8_t flags = 0;
        for (uint32_t c = 0; c < cutCount[i]; ++c, ++rec) {
            for (uint32_t q = 0; q < 2 * G; ++q) row[q] = rows[size_t(rec) * 2 * G + q] - (h->method == LC_DESENS_MD5 ? int32_t(S.from) : 0);
            lcdesens::collectStep(P, h->rewrite.refGroup.data(), true, off[i + 1] - off[i], lcdesens::kStatusMatch, row.data(), S, rec,
                                  recs.data() + size_t(rec) * W, flags);
        }
        last[i] = S.last;
    }
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (last[i] == lcdesens::kNone) continue;
        const uint32_t len = off[i + 1] - off[i];
        const uint64_t total = lcdesens::outLen(P, len, last[i], recs.data());
        lcdesens::writeValue(P, data + off[i], len, out + at, uint32_t(total), last[i], recs.data(), 0, 1);
        at += total;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (seconds) *seconds = double(t1.tv_sec - t0.tv_sec) + double(t1.tv_nsec - t0.tv_nsec) * 1e-9;
    return at;
}
void dd_fail_next_trips(int n) { gFailNext = n; }
void dd_give_up_every(int k) { gGiveUpEvery = k; }
uint64_t dd_apply_calls(void) { return gApplyCalls; }

// fixture JSON in -> lc_desensitize_process_native -> fixture JSON out (malloc'ed; dd_free).  rc_out: the processor's return code.
// view_inside: 1 when every SourceKey value of the group afterwards is unchanged text (the caller knows); set to whether the FIRST log
// event's `key` value still lies where it lay before the call
char* dd_process_json_rc(lc_desensitize_t* p, const char* groupJson, const char* key, int* rc_out, int* first_view_kept, char* err, size_t errcap) {
    logtail::PipelineEventGroup group(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!group.FromJsonString(groupJson, &error)) {
        std::snprintf(err, errcap, "%s", error.c_str());
        return nullptr;
    }
    const char* before = nullptr;
    for (auto& e : group.MutableEvents())
        if (e.Is<logtail::LogEvent>() && e.Cast<logtail::LogEvent>().HasContent(key)) {
            before = e.Cast<logtail::LogEvent>().GetContent(key).data();
            break;
        }
    *rc_out = lc_desensitize_process_native(p, &group);
    if (first_view_kept) {
        *first_view_kept = 0;
        for (auto& e : group.MutableEvents())
            if (e.Is<logtail::LogEvent>() && e.Cast<logtail::LogEvent>().HasContent(key)) {
                *first_view_kept = e.Cast<logtail::LogEvent>().GetContent(key).data() == before;
                break;
            }
    }
    return strdup(group.ToJsonString().c_str());
}
void* lc_group_native(lc_event_group_t*) { return nullptr; }  // (the fixture wrapper of c_processor_slot.cpp is not part of this build)
void dd_free(void* p) { std::free(p); }
void lc_free(void* p) { std::free(p); }
}  // extern "C"
