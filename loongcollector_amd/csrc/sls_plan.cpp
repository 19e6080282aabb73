// sls_plan.cpp -- the host-only part of the SLS encoder (include/sls/lc_sls.h): the plan's tables and the group's tags.  No HIP: the
// tests' host double links it as it is.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "sls_plan.hpp"

namespace {
void setErr(char* err, size_t errcap, const std::string& text) {
    if (err && errcap) std::snprintf(err, errcap, "%s", text.c_str());
}
void putVarint(std::vector<uint8_t>& out, uint32_t v) {
    while (v >= 0x80u) {
        out.push_back(uint8_t(v | 0x80u));
        v >>= 7;
    }
    out.push_back(uint8_t(v));
}
}  // namespace

extern "C" int lc_sls_plan_create(const char* const* keys, const uint32_t* key_len, uint32_t n_keys, const uint32_t* matched_items, uint32_t n_matched,
                                  const uint32_t* unmatched_items, uint32_t n_unmatched, lc_sls_plan_t** out, char* err, size_t errcap) {
    if (!out) return LC_ERR_ARG;
    *out = nullptr;
    if ((n_keys && (!keys || !key_len)) || (n_matched && !matched_items) || (n_unmatched && !unmatched_items)) return LC_ERR_ARG;
    if (n_matched > LC_SLS_MAX_ITEMS || n_unmatched > LC_SLS_MAX_ITEMS) {
        setErr(err, errcap, "an item list of more than " + std::to_string(LC_SLS_MAX_ITEMS) + " items");
        return LC_ERR_UNSUPPORTED;
    }
    uint64_t keyBytes = 0;
    for (uint32_t k = 0; k < n_keys; ++k) keyBytes += key_len[k];
    if (keyBytes > LC_SLS_MAX_KEY_BYTES) {
        setErr(err, errcap, "more than " + std::to_string(LC_SLS_MAX_KEY_BYTES) + " bytes of keys");
        return LC_ERR_UNSUPPORTED;
    }
    auto plan = std::make_unique<lc_sls_plan>();
    plan->nMatched = n_matched;
    plan->nUnmatched = n_unmatched;
    // one prefix per key, shared by the items that name it
    std::vector<uint32_t> prefixAt(n_keys), prefixLen(n_keys);
    for (uint32_t k = 0; k < n_keys; ++k) {
        while (plan->blob.size() & 3u) plan->blob.push_back(0);
        prefixAt[k] = uint32_t(plan->blob.size());
        plan->blob.push_back(0x0A);
        putVarint(plan->blob, key_len[k]);
        plan->blob.insert(plan->blob.end(), keys[k], keys[k] + key_len[k]);
        plan->blob.push_back(0x12);
        prefixLen[k] = uint32_t(plan->blob.size()) - prefixAt[k];
    }
    while (plan->blob.empty() || (plan->blob.size() & 15u)) plan->blob.push_back(0);
    for (int list = 0; list < 2; ++list) {
        const uint32_t* items = list ? unmatched_items : matched_items;
        const uint32_t count = list ? n_unmatched : n_matched;
        bool anyGroup = false;
        plan->boundFixed[list] = 1 + 3 + 6 + 5;  // 0x0A varint(logSZ < 2^21) 0x08 varint5 [0x25 fixed32]
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t key = items[2 * j], source = items[2 * j + 1];
            if (key >= n_keys) {
                setErr(err, errcap, "an item names key " + std::to_string(key) + " of " + std::to_string(n_keys));
                return LC_ERR_ARG;
            }
            plan->items.push_back(lcsls::SlsItem{prefixAt[key], prefixLen[key], source, 0});
            if (source > plan->maxSource) plan->maxSource = source;
            plan->boundFixed[list] += 1 + 2 + prefixLen[key] + 2;  // 0x12 varint(csz < 2^14) prefix varint(vlen < 2^14)
            if (source == 0) ++plan->boundLines[list];
            else anyGroup = true;
        }
        if (anyGroup) ++plan->boundLines[list];
    }
    if (plan->items.empty()) plan->items.push_back(lcsls::SlsItem{0, 0, 0, 0});  // (never read: both lists are empty)
    *out = plan.release();
    return LC_OK;
}

extern "C" void lc_sls_plan_free(lc_sls_plan_t* plan) {
    if (!plan) return;
    if (plan->releaseDevice) plan->releaseDevice(plan);
    delete plan;
}

// AddTopic / AddSource / AddMachineUUID / AddLogTag, LogGroupSerializer.cpp:145-183; the order is the caller's
extern "C" int lc_sls_append_tags(const char* const* keys, const uint32_t* key_len, const char* const* values, const uint32_t* value_len, uint32_t n,
                                  uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!out_len || (n && (!keys || !key_len || !values || !value_len))) return LC_ERR_ARG;
    std::vector<uint8_t> bytes;
    for (uint32_t i = 0; i < n; ++i) {
        const std::string key(keys[i], key_len[i]);
        const uint8_t field = key == "__topic__" ? 0x1A : key == "__source__" ? 0x22 : key == "__machine_uuid__" ? 0x2A : 0;
        if (field) {
            bytes.push_back(field);
            putVarint(bytes, value_len[i]);
            bytes.insert(bytes.end(), values[i], values[i] + value_len[i]);
            continue;
        }
        bytes.push_back(0x32);
        putVarint(bytes, 1 + lcsls::varintSize(key_len[i]) + key_len[i] + 1 + lcsls::varintSize(value_len[i]) + value_len[i]);
        bytes.push_back(0x0A);
        putVarint(bytes, key_len[i]);
        bytes.insert(bytes.end(), keys[i], keys[i] + key_len[i]);
        bytes.push_back(0x12);
        putVarint(bytes, value_len[i]);
        bytes.insert(bytes.end(), values[i], values[i] + value_len[i]);
    }
    *out_len = bytes.size();
    if (bytes.size() > out_cap) return LC_ERR_OVERFLOW;
    if (!bytes.empty()) {
        if (!out) return LC_ERR_ARG;
        std::memcpy(out, bytes.data(), bytes.size());
    }
    return LC_OK;
}
