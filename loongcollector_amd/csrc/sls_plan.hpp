// sls_plan.hpp -- the plan of the SLS encoder (include/sls/lc_sls.h): what an event becomes, as the item lists sls_vm.hpp reads.
// Built on the host (sls_plan.cpp, no HIP); sls_device.hip keeps a copy per device.
#pragma once

#include <mutex>
#include <vector>

#include "../../include/sls/lc_sls.h"
#include "sls_vm.hpp"

struct lc_sls_plan {
    std::vector<uint8_t> blob;          // per item `0x0A varint(klen) key 0x12`, each 4-byte aligned
    std::vector<lcsls::SlsItem> items;  // the matched list, then the unmatched one
    uint32_t nMatched = 0, nUnmatched = 0;
    uint32_t maxSource = 0;             // the highest capture group an item names
    // a record's bytes for a line of L bytes whose rows do not overlap are at most fixed + lines * L (per list: matched, unmatched)
    uint64_t boundFixed[2] = {0, 0}, boundLines[2] = {0, 0};

    lcsls::SlsPlanView hostView() const { return lcsls::SlsPlanView{blob.data(), items.data(), nMatched, nUnmatched}; }

    // the copies sls_device.hip made: one block per device (items, then the blob), released through `releaseDevice`
    struct OnDevice {
        int dev;
        void* block;
    };
    std::mutex mu;
    std::vector<OnDevice> onDevice;
    void (*releaseDevice)(lc_sls_plan*) = nullptr;
};
