// tests/native/strrep_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main, run as a child process, plain and
// under AddressSanitizer + UBSan) that walks the per-value routines of csrc/strrep_vm.hpp -- the functions the kernels run per lane,
// compiled here for the host -- over the cases on its standard input:
//     "<method> <len(Match)> <len(ReplaceString)> <len(value)>\n" Match ReplaceString value "\n"         (method: 0 const, 1 unquote)
// and prints per case "<flags> <output bytes as hex, or - without CHANGED>\n".  Every value is walked at all 16 alignments of its first
// byte, from an exactly-sized heap copy (a read behind it is an out-of-bounds read), the size pass first (flags, length, one record per
// unit), then the write pass unit by unit from the records alone, last unit first, into an exactly-sized block.  A case whose
// alignments disagree among themselves prints "DIFFER <head>" instead.  The comparison with the model is the caller's
// (tests/helpers/strrep_cases.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../loongcollector_amd/csrc/strrep_vm.hpp"

int main() {
    char header[128];
    while (std::fgets(header, sizeof header, stdin)) {
        unsigned method = 0, ml = 0, rl = 0, vl = 0;
        if (std::sscanf(header, "%u %u %u %u", &method, &ml, &rl, &vl) != 4 || ml > LC_STRREP_MAX_MATCH || rl > LC_STRREP_MAX_REPLACE) return 2;
        StrrepConfig cfg{};
        cfg.method = method;
        cfg.matchLen = ml;
        cfg.replLen = rl;
        if (ml && std::fread(cfg.match, 1, ml, stdin) != ml) return 2;
        if (rl && std::fread(cfg.repl, 1, rl, stdin) != rl) return 2;
        std::unique_ptr<uint8_t[]> value(new uint8_t[vl ? vl : 1]);
        if (vl && std::fread(value.get(), 1, vl, stdin) != vl) return 2;
        if (std::fgetc(stdin) != '\n') return 2;
        std::string first;
        bool differ = false;
        for (uint32_t head = 0; head < 16 && !differ; ++head) {
            const uint32_t units = (head + vl + 15) / 16;
            std::unique_ptr<uint32_t[]> records(new uint32_t[units ? units : 1]);
            uint8_t flags = 0xEE;
            const uint64_t total = strrepSizeHost(cfg, value.get(), vl, head, &flags, records.get());
            std::string line = std::to_string(unsigned(flags)) + " ";
            if (flags & LC_STRREP_CHANGED) {
                std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
                std::memset(out.get(), 0xA5, total ? total : 1);
                strrepWriteHost(cfg, value.get(), vl, head, records.get(), out.get(), total);
                static const char* hex = "0123456789abcdef";
                for (uint64_t i = 0; i < total; ++i) {
                    line += hex[out[i] >> 4];
                    line += hex[out[i] & 15];
                }
                if (total == 0) line += "=";  // (changed, to zero bytes)
            } else {
                line += "-";
                if (total != 0) line += "!";
            }
            if (head == 0) first = line;
            else if (line != first) {
                std::printf("DIFFER %u %s | %s\n", head, first.c_str(), line.c_str());
                differ = true;
            }
        }
        if (!differ) std::printf("%s\n", first.c_str());
    }
    return 0;
}
