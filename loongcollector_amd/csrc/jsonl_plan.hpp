// jsonl_plan.hpp -- the plan of the JSON-lines encoder (include/jsonl/lc_jsonl.h): what an event becomes, as the item lists
// jsonl_vm.hpp reads.  Built on the host (jsonl_plan.cpp, no HIP); jsonl_device.hip keeps a copy per device.
#pragma once

#include <mutex>
#include <vector>

#include "../../include/jsonl/lc_jsonl.h"
#include "jsonl_vm.hpp"

struct lc_jsonl_plan {
    std::vector<uint8_t> blob;              // per key `,"<escaped key cut at NUL>":"`, each 4-byte aligned
    std::vector<lcjsonl::JsonlItem> items;  // the matched list, then the unmatched one
    uint32_t nMatched = 0, nUnmatched = 0;
    uint32_t maxSource = 0;                 // the highest capture group an item names
    // a record's bytes for a line of L bytes whose rows do not overlap and hold no reactive byte are at most
    // head + fixed + lines * L (per list: matched, unmatched)
    uint64_t boundFixed[2] = {0, 0}, boundLines[2] = {0, 0};

    lcjsonl::JsonlPlanView hostView() const { return lcjsonl::JsonlPlanView{blob.data(), items.data(), nMatched, nUnmatched}; }
    uint32_t itemStride() const { return nMatched > nUnmatched ? nMatched : nUnmatched; }

    // the copies jsonl_device.hip made: one block per device (items, then the blob), released through `releaseDevice`
    struct OnDevice {
        int dev;
        void* block;
    };
    std::mutex mu;
    std::vector<OnDevice> onDevice;
    void (*releaseDevice)(lc_jsonl_plan*) = nullptr;
};
