// tests/native/codec_double.cpp -- TEST INFRASTRUCTURE ONLY: the field codec processors on a box without a GPU.
//
// csrc/processor_codec_gpu.cpp (the selector, the gather, the stitch, counters, alarms, the JSON form) asks the engine for ONE thing:
// lc_codec_apply_host.  This translation unit answers it on the CPU by running the PRODUCT's per-unit routines -- the host walks of
// csrc/codec_vm.hpp, built from the unit functions the kernels run per lane -- over a copy of each value that ends exactly at the
// value's end.  tests/helpers/codec_product.py builds processor_codec_gpu.cpp + this file into tests/_build/libcodec_double.so.  Never
// linked into loongcollector_amd/lib.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/codec/lc_codec.h"
#include "../../loongcollector_amd/csrc/processor_codec_gpu.hpp"

static uint64_t gTrips = 0, gValues = 0;
static int gFailNext = 0;

extern "C" {
int lc_device_count(void) { return 1; }
const char* lc_last_error(void) { return "the double's trip was told to fail"; }

int lc_codec_apply_host(const lc_codec_t* p, const uint8_t* const* lines, const uint32_t* len, uint32_t n, uint8_t* flags, uint32_t* err_off,
                        uint64_t* out_off, uint32_t* out_len, uint8_t** out) {
    if (out) *out = nullptr;
    if (!p || !out || !out_off) return LC_ERR_ARG;
    out_off[0] = 0;
    if (n == 0) return LC_OK;
    if (!lines || !len || !flags || !out_len) return LC_ERR_ARG;
    if (gFailNext) {
        --gFailNext;
        return LC_ERR_HIP;
    }
    ++gTrips;
    gValues += n;
    const CodecConfig& cfg = lcCodecConfig(p);
    std::vector<uint8_t> bytes;
    for (uint32_t i = 0; i < n; ++i) {
        // exactly-sized: a read behind the value is an out-of-bounds read of this heap block
        std::unique_ptr<uint8_t[]> copy(new uint8_t[len[i] ? len[i] : 1]);
        if (len[i]) std::memcpy(copy.get(), lines[i], len[i]);
        const size_t at = bytes.size();  // a multiple of 16
        flags[i] = kCodecFlagOut;
        if (cfg.op == kCodecEncode) {
            out_len[i] = codecEncodedLen(len[i]);
            bytes.resize(at + codecRound16(out_len[i]), 0xA5);
            codecEncodeHost(copy.get(), len[i], bytes.data() + at);
        } else if (cfg.op == kCodecMd5) {
            out_len[i] = 32;
            bytes.resize(at + 32, 0xA5);
            codecMd5Host(copy.get(), len[i], bytes.data() + at);
        } else {
            uint32_t where = 0;
            bool clean = false;
            flags[i] = uint8_t(codecDecodeSizeHost(copy.get(), len[i], i & 15u, &out_len[i], &where, &clean));
            if (flags[i] & kCodecFlagError) {
                if (err_off) err_off[i] = where;
            } else {
                bytes.resize(at + codecRound16(out_len[i]), 0xA5);
                codecDecodeWriteHost(copy.get(), len[i], clean, out_len[i], bytes.data() + at);
            }
        }
        out_off[i + 1] = bytes.size();
    }
    if (!bytes.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(bytes.size()));
        if (!*out) return LC_ERR_ARG;
        std::memcpy(*out, bytes.data(), bytes.size());
    }
    return LC_OK;
}
void cd_fail_next_trips(int n) { gFailNext = n; }
// trips, values over all trips
void cd_trip_stats(uint64_t out[2]) {
    out[0] = gTrips;
    out[1] = gValues;
}
}  // extern "C"
