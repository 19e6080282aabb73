// tests/native/prom_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main) that walks lines through
// promParseLine() / promFinishHost() / promUnescape() of csrc/prom_vm.hpp from exactly-sized heap buffers.  tests/test_prom_host.py
// builds it with -fsanitize=address,undefined and runs it as a child process: a read behind a line's end (the backslash as the last
// byte), a label entry written behind W, or a signed overflow in the number accumulators ends it with a report.
// Input (stdin): per line honor_timestamps (0 / 1), a blank, a decimal length, a newline, that many bytes, a newline.
// Output: per line "status flags nb ne bits vb ve tb te secs nanos nlabels unescaped_bytes" of the finished walk at head 0, W = 64.
// The walks at heads 7 and 15 and at W = 1 must give the same fields (exit 3 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../loongcollector_amd/csrc/prom_vm.hpp"

static bool sameFields(const PromLine& a, const PromLine& b) {
    return a.status == b.status && a.flags == b.flags && a.name.begin == b.name.begin && a.name.end == b.name.end && a.value == b.value &&
           a.valueSpan.begin == b.valueSpan.begin && a.valueSpan.end == b.valueSpan.end && a.timeSpan.begin == b.timeSpan.begin &&
           a.timeSpan.end == b.timeSpan.end && a.secs == b.secs && a.nanos == b.nanos && a.nlabels == b.nlabels;
}

int main() {
    unsigned long honor = 0, len = 0, lines = 0;
    constexpr uint32_t kWide = 64;
    while (std::scanf("%lu %lu", &honor, &len) == 2) {
        if (std::getchar() != '\n') return 2;
        uint8_t* line = static_cast<uint8_t*>(std::malloc(len ? len : 1));
        if (len && std::fread(line, 1, len, stdin) != len) return 2;
        if (std::getchar() != '\n') return 2;
        PromLine first;
        for (uint32_t head : {0u, 7u, 15u}) {
            for (uint32_t W : {kWide, 1u}) {
                int32_t* labels = static_cast<int32_t*>(std::malloc(size_t(W) * 16));  // exactly W entries
                PromLine r;
                promParseLineHost(line, uint32_t(len), honor != 0, labels, W, r, head);
                promFinishHost(line, r);
                for (const PromSpan s : {r.name, r.valueSpan, r.timeSpan})
                    if (s.begin < 0 || s.begin > s.end || uint32_t(s.end) > len) return 3;
                size_t unescaped = 0;
                for (uint32_t k = 0; k < r.nlabels && k < W; ++k) {
                    const int32_t* l = labels + size_t(k) * 4;
                    const int32_t vb = int32_t(uint32_t(l[2]) & ~LC_PROM_LABEL_ESCAPED);
                    if (l[0] < 0 || l[0] >= l[1] || l[1] > vb || vb > l[3] || uint32_t(l[3]) >= len) return 3;
                    if (uint32_t(l[2]) & LC_PROM_LABEL_ESCAPED) {
                        std::string text;
                        promUnescape(line, vb, l[3], text);
                        unescaped += text.size();
                    }
                }
                if (head == 0u && W == kWide) {
                    first = r;
                    std::printf("%u %u %d %d %016llx %d %d %d %d %lld %u %u %zu\n", unsigned(r.status), unsigned(r.flags), r.name.begin, r.name.end,
                                static_cast<unsigned long long>(r.value), r.valueSpan.begin, r.valueSpan.end, r.timeSpan.begin, r.timeSpan.end,
                                static_cast<long long>(r.secs), r.nanos, r.nlabels, unescaped);
                } else if (!sameFields(r, first)) {
                    return 3;
                }
                std::free(labels);
            }
        }
        std::free(line);
        ++lines;
    }
    std::fprintf(stderr, "%lu lines\n", lines);
    return 0;
}
