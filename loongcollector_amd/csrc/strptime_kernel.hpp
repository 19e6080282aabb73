// strptime_kernel.hpp -- strptime_kernel: the timestamp parser on gfx950 (wave64), included by timestamp_device.hip only.
//
// One value per lane, strptimeRun() of strptime_vm.hpp per lane.
//   * the program (at most kStrptimeMaxOps words) and the name block (480 bytes) are copied into LDS once per workgroup; the routine's
//     program counter does not depend on the value, so an op fetch is one LDS read at a wave-uniform address (a broadcast), and the
//     name bytes are read the same way by the lanes that stand in the same name.
//   * a value is addressed as the capture table addresses it: base + line offset + (begin, end) of the span.  A lane reads its value
//     through ALIGNED dword loads and keeps the last one (a value is ~30 bytes: eight loads, each byte fetched once while the walk
//     goes forward); a load never leaves the 4-byte unit a byte of the value lies in -- inside the contract of lc_regex_gpu.h for d_data.
//   * same_as_prev needs the predecessor's result: a workgroup of 256 lanes covers 255 NEW values and parses the one before them again
//     in lane 0 (1/256 more work, no second launch, no cross-workgroup traffic).  Lane t reads what lane t - 1 found from LDS and, when
//     both parsed and their matched prefixes (matched minus the %f digits) have one length, compares the two prefixes' bytes.
//   * results: one status byte, int64 seconds, 32-bit nanoseconds, matched length, %f length, same_as_prev -- plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

#include "strptime_vm.hpp"

namespace lcts {

constexpr int kBlock = 256;
constexpr int kNewPerBlock = kBlock - 1;

struct Outputs {
    uint8_t* status;
    int64_t* secs;
    uint32_t* nanos;
    int32_t* matched;
    int32_t* fracLen;
    uint8_t* sameAsPrev;
};
// where the values are: value i = data[off[i] + spans[i * stride + col] .. off[i] + spans[i * stride + col + 1]); lineStatus (optional):
// the parser's status byte of line i, a value exists where it equals `matchValue`
struct Values {
    const uint8_t* data;
    const uint32_t* off;
    const int32_t* spans;
    uint32_t stride, col;
    const uint8_t* lineStatus;
    uint32_t matchValue;
};

struct GlobalDwordSource {
    const uint8_t* base;  // the value's first byte
    mutable uintptr_t haveAt;
    mutable uint32_t have;
    __device__ __forceinline__ explicit GlobalDwordSource(const uint8_t* b) : base(b), haveAt(~uintptr_t(0)), have(0) {}
    __device__ __forceinline__ uint32_t at(uint32_t i) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(base) + i, w = a & ~uintptr_t(3);
        if (w != haveAt) {
            have = *reinterpret_cast<const uint32_t*>(w);
            haveAt = w;
        }
        return (have >> ((a & 3u) * 8)) & 255u;
    }
};

// the name block is the same for every format: one object in constant memory, not a kernel argument
__constant__ StrptimeNames kDeviceNames = lcts_detail::makeNames();

__global__ __launch_bounds__(kBlock) void strptime_kernel(StrptimeProgram prog, Values v, uint32_t n, Outputs out) {
    __shared__ uint32_t sProg[kStrptimeMaxOps];
    __shared__ uint8_t sNames[kTsNameBytes];
    __shared__ uint32_t sPrefix[kBlock];   // bit 31: parsed; low bits: the matched prefix's length
    __shared__ uint64_t sAddr[kBlock];     // the value's first byte
    const uint32_t tid = threadIdx.x;
    if (tid < kStrptimeMaxOps) sProg[tid] = prog.words[tid];
    for (uint32_t i = tid; i < kTsNameBytes; i += kBlock) sNames[i] = kDeviceNames.b[i];
    __syncthreads();
    // lane 0 repeats the last value of the workgroup before; lane t > 0 owns value blockIdx * 255 + t - 1
    const int64_t idx = int64_t(blockIdx.x) * kNewPerBlock + int64_t(tid) - 1;
    const bool live = idx >= 0 && idx < int64_t(n);
    const uint8_t* p = v.data;
    uint32_t len = 0;
    bool present = false;
    if (live) {
        const size_t at = size_t(idx) * v.stride + v.col;
        const int32_t b = v.spans[at], e = v.spans[at + 1];
        present = b >= 0 && e >= b && (!v.lineStatus || v.lineStatus[idx] == v.matchValue);
        if (present) {
            p = v.data + v.off[idx] + uint32_t(b);
            len = uint32_t(e - b);
        }
    }
    StrptimeResult r;
    r.status = LC_TS_ABSENT;
    r.secs = 0;
    r.nanos = 0;
    r.matched = 0;
    r.fracLen = 0;
    typedef __attribute__((address_space(3))) const uint32_t* LdsWords;
    typedef __attribute__((address_space(3))) const uint8_t* LdsBytes;
    if (present) {
        GlobalDwordSource src(p);
        r = strptimeRun(src, len, (LdsWords)sProg, prog.n, (LdsBytes)sNames);
    }
    const uint32_t prefix = uint32_t(r.matched - r.fracLen);
    sPrefix[tid] = ((r.status & LC_TS_OK) ? 0x80000000u : 0u) | prefix;
    sAddr[tid] = uint64_t(reinterpret_cast<uintptr_t>(p));
    __syncthreads();
    if (tid == 0 || !live) return;
    uint8_t same = 0;
    const uint32_t before = sPrefix[tid - 1];
    if ((r.status & LC_TS_OK) && before == (0x80000000u | prefix)) {
        GlobalDwordSource mine(p), theirs(reinterpret_cast<const uint8_t*>(uintptr_t(sAddr[tid - 1])));
        same = 1;
        for (uint32_t i = 0; i < prefix; ++i)
            if (mine.at(i) != theirs.at(i)) {
                same = 0;
                break;
            }
    }
    out.status[idx] = r.status;
    out.secs[idx] = r.secs;
    out.nanos[idx] = r.nanos;
    out.matched[idx] = r.matched;
    out.fracLen[idx] = r.fracLen;
    out.sameAsPrev[idx] = same;
}

}  // namespace lcts
