// tests/native/kv_double.cpp -- TEST INFRASTRUCTURE ONLY: processor_split_key_value on a box without a GPU.
//
// csrc/processor_split_key_value_gpu.cpp (Init, the gather, the mop-up trip, the stitch, counters, alarms, the JSON form) asks the engine
// for ONE thing: lc_kvsplit_host.  This translation unit answers it on the CPU by running the PRODUCT's per-value routine --
// kvSplitLine() of csrc/kv_vm.hpp, the function the kernel runs per lane, compiled here for the host -- over a copy of each value that
// ends exactly at the value's end.  tests/helpers/kv_product.py builds processor_split_key_value_gpu.cpp + this file into
// tests/_build/libkv_double.so.  Never linked into loongcollector_amd/lib.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/kvsplit/lc_kvsplit.h"
#include "../../loongcollector_amd/csrc/processor_split_key_value_gpu.hpp"

static uint64_t gTrips = 0, gValues = 0, gLastW = 0;
static int gFailNext = 0;

extern "C" {
int lc_device_count(void) { return 1; }
const char* lc_last_error(void) { return "the double's trip was told to fail"; }

int lc_kvsplit_host(const lc_kvsplit_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint32_t W, uint8_t* status, uint32_t* npairs,
                    int32_t* pairs) {
    if (!p) return LC_ERR_ARG;
    if (n == 0) return LC_OK;
    if (!lines || !len || !status || !npairs || (W && !pairs)) return LC_ERR_ARG;
    if (gFailNext) {
        --gFailNext;
        return LC_ERR_HIP;
    }
    ++gTrips;
    gValues += n;
    gLastW = W;
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the value is an out-of-bounds read of this heap block
        std::unique_ptr<uint8_t[]> copy(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copy.get(), lines[i], len[i]);
        kvSplitLineHost(lcKvConfig(p), copy.get(), len[i], i & 15u, pairs + size_t(i) * W * 4, W, &status[i], &npairs[i]);
    }
    return LC_OK;
}
void kd_fail_next_trips(int n) { gFailNext = n; }
// trips, values over all trips, W of the last trip
void kd_trip_stats(uint64_t out[3]) {
    out[0] = gTrips;
    out[1] = gValues;
    out[2] = gLastW;
}
}  // extern "C"
