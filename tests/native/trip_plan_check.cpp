// trip_plan_check.cpp -- the planning arithmetic of the packed-lines trip (csrc/trip_buffers.hpp: tripCarve, tripInLayout, tripPackLines,
// tripPackPairs, tripLayout, tripCoalesce) behind a command line, for tests/test_trip_plan.py.  Every buffer is a heap block of
// exactly the planned size, so a build with -fsanitize=address,undefined sees a write past it.  Numbers in, numbers out:
//   carve maxLines maxBytes lineResultBytes maxResultBytes cnt bytes from len...   -> ok(0|1) cnt bytes
//   inlayout payload cnt pairs(0|1)                                               -> offAt pairAt bytes
//   layout cnt elemBytes...                                                       -> bytes at...
//   pack pairs(0|1) first cnt len...     (line i is len[i] bytes of 'a' + i % 26)  -> payload, then the block in hex
//   coalesce gap b e b e ...                                                      -> moved, then b e per copy
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "trip_buffers.hpp"

static unsigned long long num(const char* s) { return std::strtoull(s, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::vector<unsigned long long> a;
    for (int i = 2; i < argc; ++i) a.push_back(num(argv[i]));
    if (what == "carve" && a.size() >= 7) {
        uint32_t cnt = uint32_t(a[4]);
        size_t bytes = size_t(a[5]);
        std::vector<uint32_t> len(a.begin() + 7, a.end());
        const bool ok = tripCarve(len.data(), uint32_t(a[6]), uint32_t(len.size()), uint32_t(a[0]), size_t(a[1]), size_t(a[2]), size_t(a[3]), &cnt, &bytes);
        std::printf("%d %u %zu\n", ok ? 1 : 0, cnt, bytes);
        return 0;
    }
    if (what == "inlayout" && a.size() == 3) {
        const TripInLayout in = tripInLayout(size_t(a[0]), uint32_t(a[1]), a[2] != 0);
        std::printf("%zu %zu %zu\n", in.offAt, in.pairAt, in.bytes);
        return 0;
    }
    if (what == "layout" && a.size() >= 1 && a.size() <= 1 + TripLayout::kMaxArrays) {
        const std::vector<size_t> each(a.begin() + 1, a.end());
        const TripLayout L = tripLayout(uint32_t(a[0]), each.data(), each.size());
        std::printf("%zu", L.bytes);
        for (size_t k = 0; k + 1 < a.size(); ++k) std::printf(" %zu", L.at[k]);
        std::printf("\n");
        return 0;
    }
    if (what == "pack" && a.size() >= 3) {
        const bool pairs = a[0] != 0;
        const uint32_t first = uint32_t(a[1]), cnt = uint32_t(a[2]);
        std::vector<uint32_t> len(a.begin() + 3, a.end());
        if (size_t(first) + cnt > len.size()) return 2;
        std::vector<uint8_t*> lines;
        size_t payload = 0;
        for (size_t i = 0; i < len.size(); ++i) {
            uint8_t* p = static_cast<uint8_t*>(std::malloc(len[i] ? len[i] : 1));
            std::memset(p, 'a' + int(i % 26), len[i]);
            lines.push_back(len[i] ? p : nullptr);  // (an empty line's pointer is never read)
            if (!len[i]) std::free(p);
            if (i >= first && i < size_t(first) + cnt) payload += len[i];
        }
        const TripInLayout in = tripInLayout(payload, cnt, pairs);
        uint8_t* block = static_cast<uint8_t*>(std::malloc(in.bytes));
        std::memset(block, 0xEE, in.bytes);
        const size_t got = tripPackLines(block, in.offAt, lines.data(), len.data(), first, cnt);
        if (pairs) tripPackPairs(block, in.pairAt, len.data(), first, cnt);
        std::printf("%zu\n", got);
        for (size_t i = 0; i < in.bytes; ++i) std::printf("%02x", block[i]);
        std::printf("\n");
        std::free(block);
        for (uint8_t* p : lines) std::free(p);
        return 0;
    }
    if (what == "coalesce" && a.size() % 2 == 1) {
        std::vector<TripRange> r, copies{TripRange{1, 2}};  // (what the list held before is dropped)
        for (size_t i = 1; i + 1 < a.size(); i += 2) r.push_back(TripRange{size_t(a[i]), size_t(a[i + 1])});
        const uint64_t moved = tripCoalesce(r.data(), r.size(), size_t(a[0]), &copies);
        std::printf("%llu", static_cast<unsigned long long>(moved));
        for (const TripRange& c : copies) std::printf(" %zu %zu", c.b, c.e);
        std::printf("\n");
        return 0;
    }
    return 2;
}
