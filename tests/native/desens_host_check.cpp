// tests/native/desens_host_check.cpp -- TEST INFRASTRUCTURE ONLY: the per-value routines of csrc/desens_vm.hpp on the host, as a
// stand-alone program meant to be built with -fsanitize=address,undefined (tests/test_desensitize_host.py does).  No Python, no regex: the
// cuts come in on stdin, one job per line
//     <method 0|1> <rewrite hex or -> <RE2 groups> <value hex or -> <cuts> <engine groups G> then per cut 2 * G offsets in the whole value
// (the engine's row: group 1 the whole match, group 2 the `before` group), and go through collectStep, outLen and writeValue from
// exactly-sized heap blocks: the value's block ends at its last byte and the output's at outLen(), so a read or a write one byte too far
// is an error the sanitizer reports.  writeValue runs twice, as one lane and as 64 lanes in turn; both must give the same bytes.
// Prints the new value in hex ("=": unchanged) per job.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../loongcollector_amd/csrc/desens_vm.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoi(s.substr(i, 2), nullptr, 16)));
    return out;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t method = 0, nCuts = 0, G = 0;
        int re2Groups = 0;
        std::string rewriteHex, valueHex;
        in >> method >> rewriteHex >> re2Groups >> valueHex >> nCuts >> G;
        const std::vector<uint8_t> rewriteBytes = unhex(rewriteHex), valueBytes = unhex(valueHex);
        const uint32_t n = uint32_t(valueBytes.size());
        std::unique_ptr<uint8_t[]> value(new uint8_t[n ? n : 1]);
        if (n) std::memcpy(value.get(), valueBytes.data(), n);
        lcdesens::ParsedRewrite R;
        if (method == lcdesens::kMethodConst) R = lcdesens::parseRewrite(std::string(rewriteBytes.begin(), rewriteBytes.end()), re2Groups);
        if (R.passThrough) {
            std::puts("=");
            continue;
        }
        const lcdesens::Program P = lcdesens::programOf(method, R);
        const uint32_t W = lcdesens::recWords(P);
        std::unique_ptr<uint32_t[]> recs(new uint32_t[size_t(nCuts ? nCuts : 1) * W]);
        lcdesens::ValueState S;
        uint8_t flags = 0;
        std::vector<int32_t> row(2 * size_t(G));
        for (uint32_t c = 0; c < nCuts; ++c) {
            for (auto& v : row) in >> v;
            if (method == lcdesens::kMethodMd5)  // a fresh search of the suffix reports offsets relative to it
                for (auto& v : row)
                    if (v >= 0) v -= int32_t(S.from);
            const bool again = lcdesens::collectStep(P, R.refGroup.data(), true, n, lcdesens::kStatusMatch, row.data(), S, c, recs.get() + size_t(c) * W, flags);
            if (S.last != c || flags || (!again && c + 1 < nCuts && !(method == lcdesens::kMethodMd5 && S.from >= n))) {
                std::fprintf(stderr, "cut %u was not taken as a cut\n", c);
                return 2;
            }
        }
        if (S.last == lcdesens::kNone) {
            std::puts("=");
            continue;
        }
        const uint64_t total = lcdesens::outLen(P, n, S.last, recs.get());
        std::unique_ptr<uint8_t[]> one(new uint8_t[total ? total : 1]), many(new uint8_t[total ? total : 1]);
        lcdesens::writeValue(P, value.get(), n, one.get(), uint32_t(total), S.last, recs.get(), 0, 1);
        for (uint32_t lane = 0; lane < 64; ++lane) lcdesens::writeValue(P, value.get(), n, many.get(), uint32_t(total), S.last, recs.get(), lane, 64);
        if (total && std::memcmp(one.get(), many.get(), size_t(total)) != 0) {
            std::fprintf(stderr, "one lane and 64 lanes wrote different bytes\n");
            return 3;
        }
        std::string hex;
        char buf[3];
        for (uint64_t i = 0; i < total; ++i) {
            std::snprintf(buf, sizeof buf, "%02x", one[i]);
            hex += buf;
        }
        std::puts(total ? hex.c_str() : "-");
    }
    return 0;
}
