// grok_plan_check.cpp -- the host planner of the speculative Grok batch (csrc/grok_plan_host.hpp: assignLevels, sortByLevel, deal,
// selectFused, decideEarly, buildChains, appendRounds, forEachQueued and the history rules) behind a command line, for
// tests/test_grok_plan_host.py.  Built with -fsanitize=address,undefined; no GPU, no library.  Numbers in, numbers out:
//   levels flat n {p cand first tableWalk}xn {p f shadow}...       -> the levels in list order; then the p's of the sorted table
//   deal used leftovers n {cost cost0 cost1 level busy}xn          -> the order; then the streams (-1: not dealt)
//   fused wideFirst maxJobs n {level cand firstNfa prepare}xn      -> the fused flags, or "stop" (prepare: 0 no, 1 yes, 2 stop)
//   early mode calibrate n {rounds reTdfa remainderSeen}xn       -> the early flags
//   chains used n {p level cand rounds anchored early cost1 ov un round0 bound}xn {p f shadow}...
//                  -> per owner "a: kind.entry.arg.list.out.count.flags ..."; then "early M covered M"; then busy, stream, owner, queued per entry
//   rounds a rounds screened                                       -> the steps of appendRounds
//   queue n {len}xn {order}xn                                      -> "owner.k" in the order the steps are queued
//   overflow seen wide | hint rounds slack ran needed | needed rounds ran word... | remainder inPlay survivors
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grok_plan_host.hpp"

using namespace grokplan;

static void printSteps(const std::vector<Step>& steps) {
    for (const Step& s : steps) std::printf(" %u.%u.%u.%u.%u.%u.%u", s.kind, s.entry, s.arg, s.list, s.out, s.count, s.flags);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::vector<unsigned long long> a;
    for (int i = 2; i < argc; ++i) a.push_back(std::strtoull(argv[i], nullptr, 10));
    size_t at = 0;
    auto next = [&]() -> unsigned long long {
        if (at >= a.size()) std::exit(2);
        return a[at++];
    };
    std::vector<uint32_t> words(PW_WORDS, 0);
    auto shadowTriples = [&] {
        while (at + 3 <= a.size()) {
            const size_t p = next(), f = next();
            words[PW_SHADOW + p * 64 + f] = uint32_t(next());
        }
    };
    if (what == "levels") {
        Knobs k;
        k.flat = next() != 0;
        std::vector<Entry> act(next());
        for (Entry& e : act) {
            e.p = uint32_t(next());
            e.cand = words[PW_CAND + e.p] = uint32_t(next());
            words[PW_FIRST + e.p] = uint32_t(next());
            e.tableWalk = next() != 0;
        }
        shadowTriples();
        assignLevels(act.data(), act.size(), words.data(), k);
        for (const Entry& e : act) std::printf(" %u", e.level);
        std::printf("\n%u:", sortByLevel(act));
        for (const Entry& e : act) std::printf(" %u", e.p);
        std::printf("\n");
        return 0;
    }
    if (what == "deal") {
        const uint32_t used = uint32_t(next());
        const bool leftovers = next() != 0;
        std::vector<Entry> act(next());
        for (Entry& e : act) {
            e.cost = double(next());
            e.cost0 = double(next());
            e.cost1 = double(next());
            e.level = uint32_t(next());
            e.busy = next() != 0;
            e.stream = -1;
        }
        uint8_t order[kMaxEntries];
        deal(act.data(), act.size(), used, leftovers, order);
        for (size_t i = 0; i < act.size(); ++i) std::printf(" %u", order[i]);
        std::printf("\n");
        for (const Entry& e : act) std::printf(" %d", e.stream);
        std::printf("\n");
        return 0;
    }
    if (what == "fused") {
        Knobs k;
        k.wideFirst = int(next());
        const size_t maxJobs = next();
        std::vector<Entry> act(next());
        std::vector<int> prepare;
        for (Entry& e : act) {
            e.level = uint32_t(next());
            e.cand = uint32_t(next());
            e.firstNfa = next() != 0;
            prepare.push_back(int(next()));
        }
        if (!selectFused(act.data(), act.size(), k, maxJobs, [&](size_t i) { return prepare[i] == 2 ? -1 : prepare[i]; })) {
            std::printf("stop\n");
            return 0;
        }
        for (const Entry& e : act) std::printf(" %d", e.fused ? 1 : 0);
        std::printf("\n");
        return 0;
    }
    if (what == "early") {
        Knobs k;
        k.earlyRounds = int(next());
        const bool calibrate = next() != 0;
        std::vector<Entry> act(next());
        for (Entry& e : act) {
            e.rounds = uint32_t(next());
            e.reTdfa = next() != 0;
            e.remainderSeen = next() != 0;
        }
        decideEarly(act.data(), act.size(), k, calibrate);
        for (const Entry& e : act) std::printf(" %d", e.early ? 1 : 0);
        std::printf("\n");
        return 0;
    }
    if (what == "chains") {
        const uint32_t used = uint32_t(next());
        std::vector<Entry> act(next());
        std::vector<uint32_t> cnt(act.size() * CW_WORDS, 0);
        for (size_t i = 0; i < act.size(); ++i) {
            Entry& e = act[i];
            e.p = uint32_t(next());
            e.level = uint32_t(next());
            e.cand = uint32_t(next());
            e.rounds = uint32_t(next());
            e.anchored = next() != 0;
            e.early = next() != 0;
            e.cost1 = double(next());
            e.stream = -1;
            cnt[i * CW_WORDS + CW_OVERFLOW] = uint32_t(next());
            cnt[i * CW_WORDS + CW_UNANCHORED] = uint32_t(next());
            cnt[i * CW_WORDS + CW_ROUND0] = uint32_t(next());
            cnt[i * CW_WORDS + CW_BOUND] = uint32_t(next());
        }
        shadowTriples();
        uint8_t order[kMaxEntries];
        const Chains c = buildChains(act.data(), act.size(), words.data(), cnt.data(), used, order);
        for (size_t i = 0; i < c.of.size(); ++i) {
            std::printf("%zu:", i);
            printSteps(c.of[i]);
        }
        std::printf("early %llu covered %llu\n", c.earlyMask, c.coveredMask);
        for (const Entry& e : act) std::printf(" %d,%d,%u,%d", e.busy ? 1 : 0, e.stream, e.owner, e.queued ? 1 : 0);
        std::printf("\n");
        return 0;
    }
    if (what == "rounds") {
        Entry e;
        const size_t id = next();
        e.rounds = uint32_t(next());
        std::vector<Step> steps;
        appendRounds(e, id, next() != 0, steps);
        printSteps(steps);
        return e.queued ? 0 : 1;
    }
    if (what == "queue") {
        Chains c;
        c.of.resize(next());
        for (size_t i = 0; i < c.of.size(); ++i)
            for (size_t k = 0, len = next(); k < len; ++k) c.of[i].push_back(Step{S_TICK, uint8_t(i), uint8_t(k), 0, 0, 0, 0});
        uint8_t order[kMaxEntries];
        for (size_t i = 0; i < c.of.size(); ++i) order[i] = uint8_t(next());
        forEachQueued(c, order, [](const Step& s) { std::printf(" %u.%u", s.entry, s.arg); });
        std::printf("\n");
        return 0;
    }
    if (what == "overflow" && a.size() == 2) {
        std::printf("%u\n", nextOverflowSeen(uint32_t(a[0]), uint32_t(a[1])));
        return 0;
    }
    if (what == "hint" && a.size() == 4) {
        const RoundsHint h = nextRoundsHint(RoundsHint{uint32_t(a[0]), uint32_t(a[1])}, uint32_t(a[2]), uint32_t(a[3]));
        std::printf("%u %u\n", h.rounds, h.slack);
        return 0;
    }
    if (what == "needed" && a.size() >= 2) {
        std::vector<uint32_t> my(CW_WORDS, 0);
        for (size_t i = 2; i < a.size() && CW_ROUND0 + i - 2 < CW_WORDS; ++i) my[CW_ROUND0 + i - 2] = uint32_t(a[i]);
        std::printf("%u\n", roundsNeeded(my.data(), uint32_t(a[0]), uint32_t(a[1])));
        return 0;
    }
    if (what == "remainder" && a.size() == 2) {
        std::printf("%d\n", nextRemainderSeen(uint32_t(a[0]), uint32_t(a[1])));
        return 0;
    }
    return 2;
}
