// tests/native/anchor_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_anchor on a box without a GPU.
//
// csrc/processor_anchor_gpu.cpp (Init, the gather, the stitch, counters, alarms, the JSON form) asks the engine for ONE thing:
// lc_anchor_locate_host.  This translation unit answers it on the CPU by running the PRODUCT's per-value routine -- anchorLocate() of
// csrc/anchor_vm.hpp, the function the kernel runs per lane, compiled here for the host -- over a copy of each value that ends exactly at
// the value's end.  tests/helpers/anchor_product.py builds processor_anchor_gpu.cpp + this file into tests/_build/libanchor_double.so.
// Never linked into loongcollector_amd/lib.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/anchor/lc_anchor.h"
#include "../../loongcollector_amd/csrc/processor_anchor_gpu.hpp"

static uint64_t gTrips = 0, gValues = 0;
static int gFailNext = 0;

extern "C" {
int lc_device_count(void) { return 1; }
const char* lc_last_error(void) { return "the double's trip was told to fail"; }

int lc_anchor_locate_host(const lc_anchor_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, int32_t* spans) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !spans) return LC_ERR_ARG;
    if (gFailNext) {
        --gFailNext;
        return LC_ERR_HIP;
    }
    ++gTrips;
    gValues += n;
    const uint32_t S = anchorStride(lcAnchorConfig(p));
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the value is an out-of-bounds read of this heap block
        std::unique_ptr<uint8_t[]> copy(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copy.get(), lines[i], len[i]);
        anchorLocateHost(lcAnchorConfig(p), copy.get(), len[i], i & 15u, spans + size_t(i) * S * 2);
    }
    return LC_OK;
}
void ad_fail_next_trips(int n) { gFailNext = n; }
// trips, values over all trips
void ad_trip_stats(uint64_t out[2]) {
    out[0] = gTrips;
    out[1] = gValues;
}
}  // extern "C"
