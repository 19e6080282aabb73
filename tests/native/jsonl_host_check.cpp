// tests/native/jsonl_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main) that walks batches of events
// through jsonlRecordSize() and jsonlWriteRecordHost() of csrc/jsonl_vm.hpp -- the unit functions the kernels run per lane
// (classifyUnit, emitUnit, copyPieceLanes), composed serially and compiled here for the host -- from exactly-sized heap copies of every
// line, row, table and head into an exactly-sized output.  tests/test_jsonl_host.py builds it plain and with
// -fsanitize=address,undefined and runs it as a child process: a read outside a line or a write outside a record ends the sanitized
// build with a report.
// Input (stdin), per batch:
//   "B nkeys nmatched nunmatched nevents headlen\n" head bytes "\n"
//   per key   "klen\n" key bytes "\n"
//   per item  "key source\n"                       (the matched list, then the unmatched one)
//   per event "status time len ngroups c0 c1 ...\n" line bytes "\n"
// Output per batch: "sizes s0 s1 ...\n" and the records of the whole batch in hex ("-" when there is none).  Every batch is written at
// all 16 residues of the first record's offset, with 8 lanes and with 64; the results must be the same bytes (exit 3) and must leave the
// bytes before them alone (exit 4).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../loongcollector_amd/csrc/jsonl_vm.hpp"

namespace {
uint8_t* exact(const std::string& s) {
    uint8_t* p = static_cast<uint8_t*>(std::malloc(s.size() ? s.size() : 1));
    if (!s.empty()) std::memcpy(p, s.data(), s.size());
    return p;
}
bool readBytes(size_t n, std::string* out) {
    out->resize(n);
    if (n && std::fread(&(*out)[0], 1, n, stdin) != n) return false;
    return std::getchar() == '\n';
}
}  // namespace

int main() {
    unsigned long nkeys, nm, nu, nev, headLen, batches = 0;
    while (std::scanf(" B %lu %lu %lu %lu %lu", &nkeys, &nm, &nu, &nev, &headLen) == 5) {
        if (std::getchar() != '\n') return 2;
        std::string headText;
        if (!readBytes(headLen, &headText)) return 2;
        uint8_t* head = exact(headText);
        // the plan's tables as jsonl_plan.cpp lays them out, in exactly-sized blocks
        std::string blob;
        std::vector<uint32_t> prefixAt(nkeys), prefixLen(nkeys);
        for (unsigned long k = 0; k < nkeys; ++k) {
            unsigned long klen;
            std::string key;
            if (std::scanf("%lu", &klen) != 1 || std::getchar() != '\n' || !readBytes(klen, &key)) return 2;
            while (blob.size() & 3u) blob.push_back(0);
            prefixAt[k] = uint32_t(blob.size());
            blob += ",\"";
            lcjsonl::appendEscaped(blob, reinterpret_cast<const uint8_t*>(key.data()), key.size());
            blob += "\":\"";
            prefixLen[k] = uint32_t(blob.size()) - prefixAt[k];
        }
        uint8_t* blobCopy = exact(blob);
        const size_t nItems = nm + nu;
        lcjsonl::JsonlItem* items = static_cast<lcjsonl::JsonlItem*>(std::malloc(nItems ? nItems * sizeof(lcjsonl::JsonlItem) : 1));
        for (size_t j = 0; j < nItems; ++j) {
            unsigned long key, source;
            if (std::scanf("%lu %lu", &key, &source) != 2 || key >= nkeys) return 2;
            items[j] = lcjsonl::JsonlItem{prefixAt[key], prefixLen[key], uint32_t(source), 0};
        }
        const lcjsonl::JsonlPlanView P{blobCopy, items, uint32_t(nm), uint32_t(nu)};
        std::vector<lcjsonl::JsonlEvent> events(nev);
        std::vector<uint8_t*> lineCopies(nev);
        std::vector<int32_t*> capCopies(nev);
        std::vector<uint64_t> sizes(nev), at(nev + 1, 0);
        for (unsigned long i = 0; i < nev; ++i) {
            unsigned long status, time, len, ngroups;
            if (std::scanf("%lu %lu %lu %lu", &status, &time, &len, &ngroups) != 4) return 2;
            capCopies[i] = static_cast<int32_t*>(std::malloc(ngroups ? ngroups * 8 : 1));
            for (unsigned long g = 0; g < 2 * ngroups; ++g) {
                long c;
                if (std::scanf("%ld", &c) != 1) return 2;
                capCopies[i][g] = int32_t(c);
            }
            if (std::getchar() != '\n') return 2;
            std::string line;
            if (!readBytes(len, &line)) return 2;
            lineCopies[i] = exact(line);
            lcjsonl::JsonlEvent& e = events[i];
            e.line = lineCopies[i];
            e.lineLen = uint32_t(len);
            e.caps = capCopies[i];
            lcjsonl::eventItems(P, uint8_t(status), &e.firstItem, &e.nItems);
            e.time = uint32_t(time);
            sizes[i] = lcjsonl::jsonlRecordSize(P, e, uint32_t(headLen));
            at[i + 1] = at[i] + sizes[i];
        }
        const uint64_t total = at[nev];
        std::string first;
        for (uint32_t round = 0; round < 32; ++round) {
            const uint32_t pad = round & 15u, lanes = round < 16 ? 8 : 64;
            // 16 guard bytes in front (the buffer's own, so that the residue is the pad's), none behind: the block ends with the records
            uint8_t* out = static_cast<uint8_t*>(std::malloc(16 + pad + total));
            std::memset(out, 0xEE, 16 + pad + total);
            for (unsigned long i = 0; i < nev; ++i)
                if (sizes[i]) lcjsonl::jsonlWriteRecordHost(P, events[i], head, uint32_t(headLen), out + 16, pad + at[i], lanes);
            for (uint32_t j = 0; j < 16 + pad; ++j)
                if (out[j] != 0xEE) return 4;
            const std::string got(reinterpret_cast<const char*>(out) + 16 + pad, total);
            if (round == 0) first = got;
            else if (got != first) return 3;
            std::free(out);
        }
        std::printf("sizes");
        for (unsigned long i = 0; i < nev; ++i) std::printf(" %llu", static_cast<unsigned long long>(sizes[i]));
        std::printf("\n");
        if (first.empty()) std::printf("-");
        for (unsigned char c : first) std::printf("%02x", unsigned(c));
        std::printf("\n");
        for (unsigned long i = 0; i < nev; ++i) {
            std::free(lineCopies[i]);
            std::free(capCopies[i]);
        }
        std::free(items);
        std::free(blobCopy);
        std::free(head);
        ++batches;
    }
    std::fprintf(stderr, "%lu batches\n", batches);
    return 0;
}
