// tests/native/sls_double.cpp -- TEST INFRASTRUCTURE ONLY: lc_sls_processor_* on a box without a GPU.
//
// csrc/processor_sls_gpu.cpp (the plan read off the parser's probe events, which groups the device serves, the counters rebuilt from the
// status bytes, the copy + host writer for every other group) asks the engine for ONE thing: lc_sls_match_encode_host.  This
// translation unit answers it on the CPU: the match by the CPU oracle (tests/native/pipeline_double.cpp, which also stands in for the HIP
// runtime and answers the parser's own lc_regex_match_host_views), the records by the PRODUCT's per-event routines -- slsRecordSize()
// and slsRecordWord() of csrc/sls_vm.hpp, what the kernels run per lane, compiled here for the host -- over a copy of each line that
// ends exactly at the line's end.  tests/helpers/sls_cases.py builds c_processor_slot.cpp + processor_pipeline_gpu.cpp +
// processor_parse_regex_gpu.cpp + processor_filter_gpu.cpp + event_model.cpp + sls_plan.cpp + processor_sls_gpu.cpp + this file into
// tests/_build/libsls_double.so.  Never linked into loongcollector_amd/lib.
#include "pipeline_double.cpp"

#include <memory>

#include "../../include/sls/lc_sls.h"
#include "../../loongcollector_amd/csrc/sls_plan.hpp"

static int gSlsFailNext = 0;
static uint64_t gSlsTrips = 0;
static thread_local std::vector<uint8_t> tSlsOut;

extern "C" {
void lc_sls_thread_release(void) { tSlsOut = std::vector<uint8_t>(); }

int lc_sls_match_encode_host(lc_sls_plan_t* plan, lc_regex_t* re, const uint8_t* const* lines, const uint32_t* len, uint32_t n, const uint32_t* time,
                             const int32_t* time_ns, int enable_ns, const uint8_t** out, size_t* out_len, uint64_t* rec_off, uint8_t* status) {
    if (!plan || !re || !out || !out_len) return LC_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    if (n == 0) {
        if (rec_off) rec_off[0] = 0;
        return LC_OK;
    }
    if (!lines || !len || !time || !status || plan->maxSource > uint32_t(re->marks)) return LC_ERR_ARG;
    if (gSlsFailNext) {
        --gSlsFailNext;
        return LC_ERR_HIP;
    }
    ++gSlsTrips;
    const uint32_t G = uint32_t(re->marks);
    const lcsls::SlsPlanView P = plan->hostView();
    std::vector<int32_t> caps(size_t(n) * 2 * G), what(size_t(G + 1) * 2);
    std::vector<std::unique_ptr<uint8_t[]>> copies(n);
    std::vector<lcsls::SlsEvent> events(n);
    std::vector<uint64_t> at(size_t(n) + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the line is an out-of-bounds read of this heap block
        copies[i].reset(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copies[i].get(), lines[i], len[i]);
        matchOne(re, copies[i].get(), len[i], G, &caps[size_t(i) * 2 * G], &status[i], what);
        lcsls::SlsEvent& e = events[i];
        e.line = copies[i].get();
        e.lineLen = len[i];
        e.caps = &caps[size_t(i) * 2 * G];
        lcsls::eventItems(P, status[i], &e.firstItem, &e.nItems);
        e.time = time[i];
        e.hasNs = enable_ns && time_ns && time_ns[i] >= 0;
        e.ns = e.hasNs ? uint32_t(time_ns[i]) : 0;
        at[i + 1] = at[i] + lcsls::slsRecordSize(P, e);
    }
    tSlsOut.assign(size_t(at[n]), 0xEE);
    for (uint32_t i = 0; i < n; ++i)
        if (at[i + 1] > at[i]) lcsls::slsWriteRecordHost(P, events[i], tSlsOut.data(), at[i], uint32_t(at[i + 1] - at[i]));
    if (rec_off) std::memcpy(rec_off, at.data(), (size_t(n) + 1) * 8);
    *out = tSlsOut.data();
    *out_len = tSlsOut.size();
    return LC_OK;
}

void sd_fail_next_trips(int n) { gSlsFailNext = n; }
uint64_t sd_trips(void) { return gSlsTrips; }
}  // extern "C"
