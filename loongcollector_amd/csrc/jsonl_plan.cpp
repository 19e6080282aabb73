// jsonl_plan.cpp -- the host-only part of the JSON-lines encoder (include/jsonl/lc_jsonl.h): the plan's tables and the group's head.
// No HIP: the tests' host double links it as it is.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "jsonl_plan.hpp"

namespace {
void setErr(char* err, size_t errcap, const std::string& text) {
    if (err && errcap) std::snprintf(err, errcap, "%s", text.c_str());
}
void putText(std::vector<uint8_t>& out, const char* s) {
    while (*s) out.push_back(uint8_t(*s++));
}
}  // namespace

extern "C" int lc_jsonl_plan_create(const char* const* keys, const uint32_t* key_len, uint32_t n_keys, const uint32_t* matched_items, uint32_t n_matched,
                                    const uint32_t* unmatched_items, uint32_t n_unmatched, lc_jsonl_plan_t** out, char* err, size_t errcap) {
    if (!out) return LC_ERR_ARG;
    *out = nullptr;
    if ((n_keys && (!keys || !key_len)) || (n_matched && !matched_items) || (n_unmatched && !unmatched_items)) return LC_ERR_ARG;
    if (n_matched > LC_JSONL_MAX_ITEMS || n_unmatched > LC_JSONL_MAX_ITEMS) {
        setErr(err, errcap, "an item list of more than " + std::to_string(LC_JSONL_MAX_ITEMS) + " items");
        return LC_ERR_UNSUPPORTED;
    }
    auto plan = std::make_unique<lc_jsonl_plan>();
    plan->nMatched = n_matched;
    plan->nUnmatched = n_unmatched;
    // one prefix per key, shared by the items that name it; the bound is on the escaped bytes
    std::vector<uint32_t> prefixAt(n_keys), prefixLen(n_keys);
    uint64_t keyBytes = 0;
    for (uint32_t k = 0; k < n_keys; ++k) {
        while (plan->blob.size() & 3u) plan->blob.push_back(0);
        prefixAt[k] = uint32_t(plan->blob.size());
        putText(plan->blob, ",\"");
        const size_t before = plan->blob.size();
        lcjsonl::appendEscaped(plan->blob, reinterpret_cast<const uint8_t*>(keys[k]), key_len[k]);
        keyBytes += plan->blob.size() - before;
        if (keyBytes > LC_JSONL_MAX_KEY_BYTES) {
            setErr(err, errcap, "more than " + std::to_string(LC_JSONL_MAX_KEY_BYTES) + " bytes of escaped keys");
            return LC_ERR_UNSUPPORTED;
        }
        putText(plan->blob, "\":\"");
        prefixLen[k] = uint32_t(plan->blob.size()) - prefixAt[k];
    }
    while (plan->blob.empty() || (plan->blob.size() & 15u)) plan->blob.push_back(0);
    for (int list = 0; list < 2; ++list) {
        const uint32_t* items = list ? unmatched_items : matched_items;
        const uint32_t count = list ? n_unmatched : n_matched;
        bool anyGroup = false;
        plan->boundFixed[list] = 10 + 2;  // the time's digits, }\n
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t key = items[2 * j], source = items[2 * j + 1];
            if (key >= n_keys) {
                setErr(err, errcap, "an item names key " + std::to_string(key) + " of " + std::to_string(n_keys));
                return LC_ERR_ARG;
            }
            plan->items.push_back(lcjsonl::JsonlItem{prefixAt[key], prefixLen[key], source, 0});
            if (source > plan->maxSource) plan->maxSource = source;
            plan->boundFixed[list] += prefixLen[key] + 1;
            if (source == 0) ++plan->boundLines[list];
            else anyGroup = true;
        }
        if (anyGroup) ++plan->boundLines[list];
    }
    if (plan->items.empty()) plan->items.push_back(lcjsonl::JsonlItem{0, 0, 0, 0});  // (never read: both lists are empty)
    *out = plan.release();
    return LC_OK;
}

extern "C" void lc_jsonl_plan_free(lc_jsonl_plan_t* plan) {
    if (!plan) return;
    if (plan->releaseDevice) plan->releaseDevice(plan);
    delete plan;
}

// JsonSerializer.cpp:52-58 over SizedMap::mInner, a std::map<StringView, StringView>: ascending by key, bytes compared as unsigned, a
// shorter key before its extensions
extern "C" int lc_jsonl_head(const char* const* keys, const uint32_t* key_len, const char* const* values, const uint32_t* value_len, uint32_t n,
                             uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!out_len || (n && (!keys || !key_len || !values || !value_len))) return LC_ERR_ARG;
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    const auto cmp = [&](uint32_t a, uint32_t b) {
        const size_t common = std::min(key_len[a], key_len[b]);
        const int c = common ? std::memcmp(keys[a], keys[b], common) : 0;
        return c ? c < 0 : key_len[a] < key_len[b];
    };
    std::sort(order.begin(), order.end(), cmp);
    for (uint32_t i = 1; i < n; ++i)
        if (!cmp(order[i - 1], order[i])) return LC_ERR_ARG;  // two equal keys: a map holds none
    std::vector<uint8_t> bytes;
    bytes.push_back('{');
    for (uint32_t i : order) {
        bytes.push_back('"');
        lcjsonl::appendEscaped(bytes, reinterpret_cast<const uint8_t*>(keys[i]), key_len[i]);
        putText(bytes, "\":\"");
        lcjsonl::appendEscaped(bytes, reinterpret_cast<const uint8_t*>(values[i]), value_len[i]);
        putText(bytes, "\",");
    }
    putText(bytes, "\"__time__\":");
    *out_len = bytes.size();
    if (bytes.size() > out_cap) return LC_ERR_OVERFLOW;
    if (!out) return LC_ERR_ARG;
    std::memcpy(out, bytes.data(), bytes.size());
    return LC_OK;
}
