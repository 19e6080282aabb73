// tests/native/anchor_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main) that walks values through
// anchorLocate() of csrc/anchor_vm.hpp from exactly-sized heap buffers, through a source that answers the positions behind the value
// with the bytes that follow it in a packed buffer (held in a block of their own) and needle first bytes for everything else.
// tests/test_anchor_host.py builds it plain and with -fsanitize=address,undefined and runs it as a child process: a read outside the
// value or an entry written outside the row ends the sanitized build with a report.
// Input (stdin): per value "count len tail\n", the 2 * count needle lengths "sl0 pl0 sl1 pl1 ...\n", then the needles in that order, the
// value and the tail back to back, a newline.
// Output: per value "b0 e0 b1 e1 ..." (count entries), from the walk at head 0 into a row of exactly S entries.  The walks at the other
// 15 heads must agree with it (exit 3), the pad entry of an odd count must be (-1, -1) (exit 5).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../loongcollector_amd/csrc/anchor_vm.hpp"

int main() {
    unsigned long count = 0, len = 0, tailLen = 0, values = 0;
    while (std::scanf("%lu %lu %lu", &count, &len, &tailLen) == 3) {
        if (std::getchar() != '\n' || count > LC_ANCHOR_MAX_ANCHORS) return 2;
        unsigned long nl[2 * LC_ANCHOR_MAX_ANCHORS];
        for (unsigned long i = 0; i < 2 * count; ++i)
            if (std::scanf("%lu", &nl[i]) != 1 || nl[i] > LC_ANCHOR_MAX_NEEDLE) return 2;
        if (std::getchar() != '\n') return 2;
        AnchorConfig cfg{};
        for (unsigned long a = 0; a < count; ++a) {
            uint8_t start[LC_ANCHOR_MAX_NEEDLE], stop[LC_ANCHOR_MAX_NEEDLE];
            if (std::fread(start, 1, nl[2 * a], stdin) != nl[2 * a] || std::fread(stop, 1, nl[2 * a + 1], stdin) != nl[2 * a + 1]) return 2;
            if (!anchorAdd(&cfg, start, nl[2 * a], stop, nl[2 * a + 1])) return 2;
        }
        uint8_t* value = static_cast<uint8_t*>(std::malloc(len ? len : 1));  // exactly-sized: a read behind it is out of bounds
        uint8_t* tail = static_cast<uint8_t*>(std::malloc(tailLen ? tailLen : 1));
        if (len && std::fread(value, 1, len, stdin) != len) return 2;
        if (tailLen && std::fread(tail, 1, tailLen, stdin) != tailLen) return 2;
        if (std::getchar() != '\n') return 2;
        const uint32_t S = anchorStride(cfg);
        const size_t rowBytes = S ? size_t(S) * 8 : 1;
        int32_t* row0 = static_cast<int32_t*>(std::malloc(rowBytes));  // exactly S entries
        for (uint32_t head = 0; head < 16; ++head) {
            int32_t* row = head ? static_cast<int32_t*>(std::malloc(rowBytes)) : row0;
            std::memset(row, 0xEE, rowBytes);
            anchorLocateHost(cfg, value, uint32_t(len), head, row, tail, uint32_t(tailLen));
            if (head && S && std::memcmp(row, row0, size_t(S) * 8) != 0) return 3;
            if (head) std::free(row);
        }
        if (S > count && (row0[2 * count] != -1 || row0[2 * count + 1] != -1)) return 5;
        for (unsigned long a = 0; a < count; ++a) std::printf(a ? " %d %d" : "%d %d", row0[2 * a], row0[2 * a + 1]);
        std::printf("\n");
        std::free(row0);
        std::free(tail);
        std::free(value);
        ++values;
    }
    std::fprintf(stderr, "%lu values\n", values);
    return 0;
}
