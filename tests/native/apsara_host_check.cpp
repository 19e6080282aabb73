// tests/native/apsara_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main) that walks lines through
// apsaraParseLine() of csrc/apsara_vm.hpp from exactly-sized heap buffers.  tests/test_apsara_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process: a read behind a line's end, a signed overflow or a misaligned store in
// the routine ends it with a report.  Input (stdin): per line a decimal length, a newline, that many bytes, a newline.  Output: per
// line "status secs nanos npairs".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../loongcollector_amd/csrc/apsara_vm.hpp"

int main() {
    unsigned long len = 0;
    unsigned long lines = 0;
    while (std::scanf("%lu", &len) == 1) {
        if (std::getchar() != '\n') return 2;
        uint8_t* line = static_cast<uint8_t*>(std::malloc(len ? len : 1));
        if (len && std::fread(line, 1, len, stdin) != len) return 2;
        if (std::getchar() != '\n') return 2;
        for (uint32_t W : {0u, 1u, 400u}) {
            ApsaraPair* row = static_cast<ApsaraPair*>(std::malloc(W ? W * sizeof(ApsaraPair) : 1));
            for (uint32_t head : {0u, 7u, 15u}) {
                ApsaraLine r;
                apsaraParseHost(line, uint32_t(len), W, row, r, head);
                for (uint32_t k = 0; k < (r.npairs < W ? r.npairs : W); ++k)
                    if (row[k].keyBegin < 0 || row[k].keyBegin > row[k].colon || row[k].colon >= row[k].end || uint32_t(row[k].end) > len) return 3;
                if (W == 400u && head == 0u) std::printf("%u %lld %u %u\n", unsigned(r.status), static_cast<long long>(r.secs), r.nanos, r.npairs);
            }
            std::free(row);
        }
        std::free(line);
        ++lines;
    }
    std::fprintf(stderr, "%lu lines\n", lines);
    return 0;
}
