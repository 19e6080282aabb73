// tests/native/jsonl_double.cpp -- TEST INFRASTRUCTURE ONLY: lc_jsonl_processor_* on a box without a GPU.
//
// csrc/processor_jsonl_gpu.cpp (the plan read off the parser's probe events, the head from the group's tags, which groups the device
// serves, the counters rebuilt from the status bytes, the copy + host writer for every other group) asks the engine for ONE thing:
// lc_jsonl_match_encode_host.  This translation unit answers it on the CPU: the match by the CPU oracle (tests/native/pipeline_double.cpp,
// which also stands in for the HIP runtime and answers the parser's own lc_regex_match_host_views), the records by the PRODUCT's
// routines -- jsonlRecordSize() and jsonlWriteRecordHost() of csrc/jsonl_vm.hpp, the unit functions the kernels run per lane, compiled
// here for the host -- over a copy of each line that ends exactly at the line's end.  tests/helpers/jsonl_cases.py builds
// c_processor_slot.cpp + processor_pipeline_gpu.cpp + processor_parse_regex_gpu.cpp + processor_filter_gpu.cpp + event_model.cpp +
// jsonl_plan.cpp + processor_jsonl_gpu.cpp + this file into tests/_build/libjsonl_double.so.  Never linked into loongcollector_amd/lib.
#include "pipeline_double.cpp"

#include <memory>

#include "../../include/jsonl/lc_jsonl.h"
#include "../../loongcollector_amd/csrc/jsonl_plan.hpp"

static int gJsonlFailNext = 0;
static uint64_t gJsonlTrips = 0;
static thread_local std::vector<uint8_t> tJsonlOut;

extern "C" {
void lc_jsonl_thread_release(void) { tJsonlOut = std::vector<uint8_t>(); }

int lc_jsonl_match_encode_host(lc_jsonl_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n,
                               const uint32_t* time, const uint8_t* head, uint32_t head_len, const uint8_t** out, size_t* out_len, uint64_t* rec_off,
                               uint8_t* status) {
    if (!plan || !re || !out || !out_len) return LC_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    if (n == 0) {
        if (rec_off) rec_off[0] = 0;
        return LC_OK;
    }
    if (!lines || !len || !time || !status || !head || head_len < 12 || head_len > LC_JSONL_MAX_HEAD_BYTES) return LC_ERR_ARG;
    if (plan->maxSource > uint32_t(re->marks)) return LC_ERR_ARG;
    if (gJsonlFailNext) {
        --gJsonlFailNext;
        return LC_ERR_HIP;
    }
    ++gJsonlTrips;
    const uint32_t G = uint32_t(re->marks);
    const lcjsonl::JsonlPlanView P = plan->hostView();
    std::unique_ptr<uint8_t[]> headCopy(new uint8_t[head_len]);
    std::memcpy(headCopy.get(), head, head_len);
    std::vector<int32_t> caps(size_t(n) * 2 * G), what(size_t(G + 1) * 2);
    std::vector<std::unique_ptr<uint8_t[]>> copies(n);
    std::vector<lcjsonl::JsonlEvent> events(n);
    std::vector<uint64_t> at(size_t(n) + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the line is an out-of-bounds read of this heap block
        copies[i].reset(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copies[i].get(), lines[i], len[i]);
        matchOne(re, copies[i].get(), len[i], G, &caps[size_t(i) * 2 * G], &status[i], what);
        lcjsonl::JsonlEvent& e = events[i];
        e.line = copies[i].get();
        e.lineLen = len[i];
        e.caps = &caps[size_t(i) * 2 * G];
        lcjsonl::eventItems(P, status[i], &e.firstItem, &e.nItems);
        e.time = time[i];
        at[i + 1] = at[i] + lcjsonl::jsonlRecordSize(P, e, head_len);
    }
    tJsonlOut.assign(size_t(at[n]) + 16, 0xEE);
    uint8_t* base = tJsonlOut.data() + ((16 - (reinterpret_cast<uintptr_t>(tJsonlOut.data()) & 15u)) & 15u);  // (aligned as the device's block is)
    for (uint32_t i = 0; i < n; ++i)
        if (at[i + 1] > at[i]) lcjsonl::jsonlWriteRecordHost(P, events[i], headCopy.get(), head_len, base, at[i], 8);
    if (rec_off) std::memcpy(rec_off, at.data(), (size_t(n) + 1) * 8);
    *out = base;
    *out_len = size_t(at[n]);
    return LC_OK;
}

void jd_fail_next_trips(int n) { gJsonlFailNext = n; }
uint64_t jd_trips(void) { return gJsonlTrips; }
}  // extern "C"
