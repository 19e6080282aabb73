// tests/native/container_log_host_check.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program (its own main) that walks lines through
// clogParseContainerd() / clogParseDocker() of csrc/clog_vm.hpp from exactly-sized heap buffers.  tests/test_container_log_host.py
// builds it with -fsanitize=address,undefined and runs it as a child process: a read behind a line's end, a write of the in-place
// rewrite (or of the shadow) outside the line, or a signed overflow in the routines ends it with a report.
// Input (stdin): per line the format (1 / 2), a blank, a decimal length, a newline, that many bytes, a newline.
// Output: per line "status flags tb te sb se cb ce rewrite_begin" of the shadow walk at head 0.  The in-place walk must give the same
// fields, and its rewritten bytes must be the shadow's (exit 3 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../loongcollector_amd/csrc/clog_vm.hpp"

static bool sameFields(const ClogLine& a, const ClogLine& b) {
    return a.status == b.status && a.flags == b.flags && std::memcmp(a.span, b.span, sizeof a.span) == 0 && a.rewriteBegin == b.rewriteBegin;
}

int main() {
    unsigned long format = 0, len = 0, lines = 0;
    while (std::scanf("%lu %lu", &format, &len) == 2) {
        if (std::getchar() != '\n') return 2;
        uint8_t* line = static_cast<uint8_t*>(std::malloc(len ? len : 1));
        if (len && std::fread(line, 1, len, stdin) != len) return 2;
        if (std::getchar() != '\n') return 2;
        ClogLine first;
        for (uint32_t head : {0u, 7u, 15u}) {
            ClogLine r;
            if (format == LC_CLOG_CONTAINERD) {
                clogParseContainerdHost(line, uint32_t(len), r, head);
            } else {
                uint8_t* shadow = static_cast<uint8_t*>(std::malloc(len ? len : 1));
                uint8_t* inPlace = static_cast<uint8_t*>(std::malloc(len ? len : 1));
                std::memset(shadow, 0xA5, len ? len : 1);
                if (len) std::memcpy(inPlace, line, len);
                clogParseDockerHost(line, uint32_t(len), shadow, r, head);
                ClogLine again;
                clogParseDockerHost(inPlace, uint32_t(len), inPlace, again, head);
                if (!sameFields(r, again)) return 3;
                // a line that needs no replay: the in-place bytes of [rewrite_begin, content end) are the shadow's, and the shadow is
                // untouched outside the rewritten values
                if (r.status != LC_CLOG_FAIL_JSON && (r.flags & (LC_CLOG_ESCAPED | LC_CLOG_REPLAY)) == LC_CLOG_ESCAPED) {
                    const int32_t from = r.rewriteBegin, to = r.span[LC_CLOG_SPAN_CONTENT].end;
                    if (from <= 0 || to < from || uint32_t(to) > len || std::memcmp(shadow + from, inPlace + from, size_t(to - from)) != 0) return 3;
                    for (int32_t p = 0; p < from; ++p)
                        if (shadow[p] != 0xA5 || inPlace[p] != line[p]) return 3;
                }
                if (!(r.flags & LC_CLOG_ESCAPED))
                    for (unsigned long p = 0; p < len; ++p)
                        if (shadow[p] != 0xA5 || inPlace[p] != line[p]) return 3;
                std::free(shadow);
                std::free(inPlace);
            }
            for (int k = 0; k < 3; ++k)
                if (r.span[k].begin < 0 || r.span[k].begin > r.span[k].end || uint32_t(r.span[k].end) > len) return 3;
            if (head == 0u) {
                first = r;
                std::printf("%u %u %d %d %d %d %d %d %d\n", unsigned(r.status), unsigned(r.flags), r.span[0].begin, r.span[0].end, r.span[1].begin,
                            r.span[1].end, r.span[2].begin, r.span[2].end, r.rewriteBegin);
            } else if (!sameFields(r, first)) {
                return 3;
            }
        }
        std::free(line);
        ++lines;
    }
    std::fprintf(stderr, "%lu lines\n", lines);
    return 0;
}
