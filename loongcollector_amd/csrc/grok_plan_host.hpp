// grok_plan_host.hpp -- the host's decisions about a speculative Grok batch, as plain functions over plain data (the plan words of
// phase 1, the entries' facts and costs, the knobs, the entries' counter words): no HIP header, no environment, no I/O.
// grok_device.hip turns the answers into launches; tests/native/grok_plan_check.cpp runs them on the CPU.  `E* act`: grokplan::Entry
// or a struct derived from it (the matcher's PlanEntry adds the entry's device pointers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace grokplan {

constexpr uint32_t kMaxEntries = 64;
constexpr uint32_t kMaxStreams = 16;
// the plan words: [64] candidates of entry p | [64] values whose FIRST candidate entry is p | [64][64] candidates of entry p whose
// value's first candidate is entry f
enum { PW_CAND = 0, PW_FIRST = 64, PW_SHADOW = 128, PW_WORDS = 128 + 64 * 64 };
// the counter words of an entry (grok_plan_kernel.hpp GC_*: grok_device.hip asserts that the two lists agree)
enum { CW_UNANCHORED = 1, CW_ROUND0 = 2, CW_BOUND = 59, CW_WIDE = 60, CW_OVERFLOW = 61, CW_REMAINDER = 62, CW_FILTERED = 63, CW_WORDS = 64 };
constexpr uint32_t kMaxRounds = CW_BOUND - CW_ROUND0 - 1;  // search rounds that can be queued ahead per entry

// The plan's switches (each can be forced for A/B measurements and the parity tests; grok_device.hip fills one per batch).
struct Knobs {
    int wideFirst = 1;    // 0 off, 1 by the entry's history, 2 always
    int earlyRounds = 1;  // 0 off, 1 by the entry's history, 2 always
    bool flat = true;     // shadowed entries whose round 0 is a table walk are not levelled
    bool remainderLiteral = true;  // the literal index over the remainders, in front of the remainder screens
    bool remainderWon = true;      // slots of values an earlier entry has won drop out in front of the screens
    bool screenScaled = true;      // staged screen tables are staged scaled
    int fusedStage = -1;           // the fused launch stages the register programs: 0 / 1, -1 by the batch's size
    // once per process
    uint32_t streams = 0;  // overrides the handle's option
    bool trace = false;
    bool remSplit = false;  // diagnosis: one launch pair per entry for the remainder screens queued ahead
};

// Host view of one active entry of the batch: what the planner is told, then what it decides.
struct Entry {
    uint32_t p = 0, cand = 0;
    uint32_t rounds = 0;         // search rounds to queue (round 0 included), by the entry's history
    bool anchored = false;       // the entry has an anchored search: round 0 runs it, the search proper takes what it did not match
    bool firstNfa = false;       // round 0's automaton runs on the thread-list engine
    bool reTdfa = false;         // the search's automaton is a tagged DFA
    bool tableWalk = false;      // round 0 is a walk of tables in global memory (a complete automaton, or a lazy one)
    bool remainderSeen = false;  // history: most of the slots in play passed the remainder screen
    double cost = 0, cost0 = 0, cost1 = 0;  // heuristic; measured round 0 / leftovers (ns, 0 = unknown)
    // ---- decided
    uint32_t level = 0;  // 0: evaluated at once; L > 0: most of its candidates have an EARLIER candidate entry (of level < L) -- it waits
                         // for those and only looks at the values none of them has won (a general format behind specific ones)
    int stream = 0;
    bool fused = false;   // round 0 is a job of the one fused launch
    bool early = false;   // the rounds behind the first match are queued at the end of the entry's chain, unscreened
    bool busy = false;    // the entry has something to do in the chains besides screens and rounds (timed on calibration batches)
    bool queued = false;  // rounds behind the first match were queued for this entry
    uint32_t owner = 0;   // whose step list the entry's steps went to (itself; a level >= 2 entry: its shadower's owner)
};

// ------------------------------------------------------------------------------------------------ levels
// act: the active entries in list order.  An entry half of whose candidates have an earlier candidate entry waits for the entries that
// shadow a quarter of them or more (SYSLOGLINE behind CRONLOG / HTTPD_ERRORLOG; SHOREWALL behind SYSLOGLINE; COMBINEDAPACHELOG behind
// COMMONAPACHELOG): what those win it never looks at.  Results do not depend on the order -- only the work does.
// ... unless the entry's round 0 is a TABLE WALK: then looking at values an earlier entry will win costs a few microseconds of a
// wavefront each, while waiting costs the batch a host round trip and the entry's longest walk a second time (0.4 ms,
// profiles/round6_grok_timeline.txt).  Knobs::flat = false: levels for those too.
template <class E>
void assignLevels(E* act, size_t n, const uint32_t* words, const Knobs& k) {
    uint32_t levelOf[kMaxEntries] = {};
    for (size_t a = 0; a < n; ++a) {
        E& e = act[a];
        const uint32_t c = e.cand;
        const uint32_t shadowed = c - std::min(c, words[PW_FIRST + e.p]);
        e.level = 0;
        if (shadowed * 2 >= c && !(k.flat && e.tableWalk)) {
            uint32_t lv = 1;
            for (uint32_t f = 0; f < e.p; ++f)
                if (words[PW_SHADOW + e.p * 64 + f] * 4 >= c) lv = std::max(lv, levelOf[f] + 1);
            e.level = std::min(lv, 3u);
        }
        levelOf[e.p] = e.level;
    }
}
// the device table lists the entries of the first pass first (its finish kernel runs over a prefix of the table), list order kept
// inside a level  -> entries of level > 0
template <class E>
uint32_t sortByLevel(std::vector<E>& act) {
    std::stable_sort(act.begin(), act.end(), [](const E& x, const E& y) { return x.level < y.level; });
    uint32_t nSecond = 0;
    for (const E& e : act) nSecond += e.level != 0;
    return nSecond;
}

// ------------------------------------------------------------------------------------------------ streams
// Which stream an entry goes to.  A phase lasts as long as its most loaded stream, and the entries differ by a factor of ten (an
// anchored DFA over 300 values: 0.1 ms; the thread-list engine on a format with a free-text field in the middle: 3 ms): longest
// first, each to the least loaded of `used` streams.  Before the first measurement: the static estimate.  Round 0 (leftovers =
// false) deals the entries of level 0; the leftovers deal skips the idle entries and levels >= 2 (those ride behind their shadower).
// order: all entries, dearest first (ties in index order) -- the order the chains are queued in.
template <class E>
void deal(E* act, size_t n, uint32_t used, bool leftovers, uint8_t* order) {
    auto costOf = [&](size_t a) {
        const double known = leftovers ? act[a].cost1 : act[a].cost0;
        return known > 0 ? known : act[a].cost * 50.0;
    };
    for (size_t a = 0; a < n; ++a) order[a] = uint8_t(a);
    std::stable_sort(order, order + n, [&](uint8_t x, uint8_t y) { return costOf(x) > costOf(y); });
    double load[kMaxStreams] = {};
    for (size_t i = 0; i < n; ++i) {
        E& e = act[order[i]];
        if (leftovers ? (!e.busy || e.level >= 2) : e.level != 0) continue;
        uint32_t best = 0;
        for (uint32_t s = 1; s < used; ++s)
            if (load[s] < load[best]) best = s;
        e.stream = int(best);
        load[best] += costOf(order[i]) + 20000.0;  // (+ a launch)
    }
}

// ------------------------------------------------------------------------------------------------ round 0
// Which entries are jobs of the ONE fused launch of round 0: the entries of level 0, in table order, whose round 0 `prepare` can make
// a job of, maxJobs at most.  prepare(a): 1 = a job (the caller has built it), 0 = not this entry, < 0 = stop.  (Knobs::wideFirst = 2
// forces the wide kernel on the thread-list entries: A/B, parity tests.)  -> false: prepare stopped it
template <class E, class Prepare>
bool selectFused(E* act, size_t n, const Knobs& k, size_t maxJobs, Prepare prepare) {
    size_t jobs = 0;
    for (size_t a = 0; a < n && jobs < maxJobs; ++a) {
        E& e = act[a];
        e.fused = false;
        if (e.level || !e.cand) continue;
        if (k.wideFirst >= 2 && e.firstNfa) continue;
        const int r = prepare(a);
        if (r < 0) return false;
        if (r) {
            e.fused = true;
            ++jobs;
        }
    }
    return true;
}
// an entry's search rounds are queued ahead by its history (most of its remainders pass its screen; calibration batches run the screen
// for every entry, to keep that history).  Decided ONCE per batch.
template <class E>
void decideEarly(E* act, size_t n, const Knobs& k, bool calibrate) {
    for (size_t a = 0; a < n; ++a)
        act[a].early = k.earlyRounds && act[a].rounds >= 2 && act[a].reTdfa && (k.earlyRounds >= 2 || (!calibrate && act[a].remainderSeen));
}

// ------------------------------------------------------------------------------------------------ chains
// What round 0 left undone, as DATA: a step is one to three launches of one entry on its stream; grok_device.hip has the one switch
// that turns a step into launches.
enum StepKind : uint8_t {
    S_FINISH_SHADOWER,      // the values entry `arg` (active index) has won, on this entry's stream: a level >= 2 entry rides behind it
    S_SECOND_OVERFLOW,      // level 0: the second chance of round 0's automaton over the overflow list
    S_POST,                 // ... and its post step
    S_TICK,                 // calibration: the begin / end event of the entry's leftovers (flags)
    S_SEARCH_FIRST,         // the search proper over `list`, minus the values an earlier entry has won: filter + first chance
    S_SEARCH_SECOND_POST,   // ... its second chance + post step
    S_SHADOWED_FIRST,       // level > 0: every slot whose value nobody before has won -- filter + first chance of round 0's automaton
    S_SHADOWED_SECOND_POST, // ... its second chance + post step
    S_ROUND,                // search round `arg` (FindNextMatch from the end of the previous match): reads `list`, appends to `out`
    S_REMAINDER             // the remainder screens of this entry alone
};
enum ListSel : uint8_t { L_NONE, L_LISTA, L_LISTB, L_UNANCHORED, L_OVERFLOW };
enum StepFlags : uint8_t {
    F_TICK_BEGIN = 1,  // the calibration begin event goes in front of this step
    F_TICK_END = 2,
    F_GATE = 4         // the entry's last queued round: what it leaves in play goes onto the gate word
};
struct Step {
    uint8_t kind, entry;
    uint8_t arg;    // shadower (active index) or round
    uint8_t list;   // ListSel: the slots the step reads
    uint8_t out;    // ListSel: the list a round appends to
    uint8_t count;  // CW_*: the word that holds the length of `list`
    uint8_t flags;
};
struct Chains {
    std::vector<std::vector<Step>> of;     // per owner
    unsigned long long earlyMask = 0;      // active entries whose rounds were queued in this phase
    unsigned long long coveredMask = 0;    // ... whose remainder screens were (in the chain, or ahead of it)
};

// rounds 1 .. of entry a, one step per round; the list lengths stay on the device.  screened: round 1 reads the survivors of the
// remainder screen (they are on the unanchored list); else every slot in play (queued ahead)
template <class E>
void appendRounds(E& e, size_t a, bool screened, std::vector<Step>& out) {
    e.queued = true;
    for (uint32_t r = 1; r < e.rounds; ++r) {
        Step s{S_ROUND, uint8_t(a), uint8_t(r), 0, uint8_t((r & 1) ? L_LISTB : L_LISTA), 0, uint8_t(r + 1 == e.rounds ? F_GATE : 0)};
        if (r == 1) {
            s.list = screened ? L_UNANCHORED : L_LISTA;
            s.count = screened ? CW_REMAINDER : CW_ROUND0;
        } else {
            s.list = (r & 1) ? L_LISTA : L_LISTB;
            s.count = uint8_t(CW_ROUND0 + r - 1);
        }
        out.push_back(s);
    }
}

// The chain of entry a, appended to its owner's list.  cnt: the entries' counter words behind round 0 ([a * CW_WORDS + word]).
// activeOf: list index -> active index, -1 = not active.
template <class E>
void buildChain(E* act, size_t a, const uint32_t* words, const uint32_t* cnt, const int8_t* activeOf, Chains& c) {
    E& e = act[a];
    const uint32_t* my = cnt + a * CW_WORDS;
    const uint32_t level = e.level;
    const uint32_t ov = level ? 0u : my[CW_OVERFLOW];
    const uint32_t un = level ? 0u : my[CW_UNANCHORED];
    e.busy = level || ov || un;
    if (!level && !ov && !un && !e.early) {
        // nothing but remainders to screen, if that: the launch queued ahead of the host's read has done it
        if (my[CW_ROUND0] != 0) c.coveredMask |= 1ull << a;
        return;
    }
    if (level && my[CW_BOUND] == 0) {  // nothing left for it (values are only ever won, never lost)
        e.busy = false;
        return;
    }
    if (level >= 2) {  // behind its main shadower
        uint32_t best = 0, bestF = 0;
        for (uint32_t f = 0; f < e.p; ++f)
            if (words[PW_SHADOW + e.p * 64 + f] > best && activeOf[f] >= 0) {
                best = words[PW_SHADOW + e.p * 64 + f];
                bestF = f;
            }
        if (best) {
            const size_t sa = size_t(activeOf[bestF]);
            e.stream = act[sa].stream;
            e.owner = act[sa].owner;
            c.of[e.owner].push_back(Step{S_FINISH_SHADOWER, uint8_t(a), uint8_t(sa), L_NONE, L_NONE, 0, 0});
        }
    }
    std::vector<Step>& out = c.of[e.owner];
    const uint8_t id = uint8_t(a);
    // the search proper over the slots the anchored search did not match: two steps
    auto searchProper = [&] {
        out.push_back(Step{S_SEARCH_FIRST, id, 0, L_UNANCHORED, L_LISTB, CW_UNANCHORED, 0});
        out.push_back(Step{S_SEARCH_SECOND_POST, id, 0, L_LISTB, L_NONE, CW_FILTERED, 0});
    };
    if (level == 0) {
        if (ov) {  // the second chance of round 0's engine over the overflow list (the longest kernel of the phase: first), then the post step
            out.push_back(Step{S_SECOND_OVERFLOW, id, 0, L_OVERFLOW, L_NONE, CW_OVERFLOW, F_TICK_BEGIN});
            out.push_back(Step{S_POST, id, 0, L_OVERFLOW, L_NONE, CW_OVERFLOW, 0});
        } else if (un) {
            out.push_back(Step{S_TICK, id, 0, L_NONE, L_NONE, 0, F_TICK_BEGIN});
        }
        // (only when the anchored search left any value unmatched -- the host knows the count)
        if (e.anchored && un) searchProper();
    } else {
        // every slot whose value nobody before has won: the anchored search (or the search) in full, then the rest
        // (a level > 0 entry has no first-chance pass of round 0: its overflow list is free, the filter fills it)
        out.push_back(Step{S_SHADOWED_FIRST, id, 0, L_NONE, L_OVERFLOW, CW_OVERFLOW, F_TICK_BEGIN});
        out.push_back(Step{S_SHADOWED_SECOND_POST, id, 0, L_OVERFLOW, L_NONE, CW_OVERFLOW, 0});
        if (e.anchored) searchProper();
    }
    if (e.busy) out.push_back(Step{S_TICK, id, 0, L_NONE, L_NONE, 0, F_TICK_END});  // (whichever way the chain ended)
    if (e.early) {
        // An entry whose remainders mostly pass its screen gets its search rounds behind the first match queued HERE, at the end of its
        // chain, unscreened: they run in the shadow of this phase instead of in a phase of their own behind the remainder screens and
        // another host round trip.
        c.earlyMask |= 1ull << a;
        appendRounds(e, a, false, out);
    } else {
        // The remainder screens of THIS entry, here -- on its stream, as soon as its own chain is through -- instead of one launch for
        // all entries behind the join of the phase (that launch, 0.4-0.5 ms for a few hundred 4 KiB remainders of one shadowed entry,
        // sat between two host round trips on every batch's critical path).
        c.coveredMask |= 1ull << a;
        out.push_back(Step{S_REMAINDER, id, 0, L_NONE, L_NONE, 0, 0});
    }
}

// All chains of the batch.  ONE fork for all of it: the leftovers of level 0 and the entries of level 1 depend on round 0 only; an
// entry of level 2 or 3 goes behind the chain of the entry that shadows most of its candidates, on that entry's stream (stream order
// instead of a barrier per level).  Sets busy / stream / owner / queued; order: the leftovers deal's.
template <class E>
Chains buildChains(E* act, size_t n, const uint32_t* words, const uint32_t* cnt, uint32_t used, uint8_t* order) {
    Chains c;
    c.of.resize(n);
    int8_t activeOf[kMaxEntries];
    for (auto& x : activeOf) x = -1;
    uint32_t maxLevel = 0;
    for (size_t a = 0; a < n; ++a) {
        E& e = act[a];
        const uint32_t* my = cnt + a * CW_WORDS;
        activeOf[e.p] = int8_t(a);
        e.owner = uint32_t(a);
        maxLevel = std::max(maxLevel, e.level);
        e.busy = e.level ? my[CW_BOUND] != 0 : (my[CW_OVERFLOW] || my[CW_UNANCHORED]);
    }
    deal(act, n, used, true, order);
    for (uint32_t level = 0; level <= maxLevel; ++level)
        for (size_t i = 0; i < n; ++i)
            if (act[order[i]].level == level) buildChain(act, order[i], words, cnt, activeOf, c);
    return c;
}

// The queue order.  The steps of all chains go out round-robin, dearest chain first: step k of every chain, in `order`, before step
// k + 1.  (Queued chain after chain -- a dozen launches each, 15-20 us a launch -- the third shadowed entry's kernel started 0.8 ms
// after the fork, behind sixty launches of other entries' mostly empty follow-up steps, and it, not the second-chance kernel, ended
// the phase.)
inline size_t longestChain(const Chains& c) {
    size_t longest = 0;
    for (const auto& l : c.of) longest = std::max(longest, l.size());
    return longest;
}
template <class Run>
void forEachQueued(const Chains& c, const uint8_t* order, Run run) {
    const size_t longest = longestChain(c);
    for (size_t k = 0; k < longest; ++k)
        for (size_t i = 0; i < c.of.size(); ++i)
            if (k < c.of[order[i]].size()) run(c.of[order[i]][k]);
}

// ------------------------------------------------------------------------------------------------ histories
// (functions from the batch's counter words to the new values; the atomics that hold them are the caller's)
// did any of the entry's values need more than 64 threads (CW_WIDE: set by the wide kernel)?  seen now = 8, else forgotten a batch at
// a time
inline uint32_t nextOverflowSeen(uint32_t seen, uint32_t wideWord) { return wideWord ? 8u : seen ? seen - 1 : 0u; }
// rounds that had any value to search (my: the entry's counter words; ran != 0: the entry went on behind its queued rounds)
inline uint32_t roundsNeeded(const uint32_t* my, uint32_t rounds, uint32_t ran) {
    uint32_t needed = 1;
    for (uint32_t r = 0; r + 1 < rounds && ran == 0; ++r)
        if (my[CW_ROUND0 + r]) needed = r + 2;
    return needed;
}
// how many rounds the entry should queue ahead next time: what this batch needed, forgotten slowly (four batches in a row that
// needed fewer)
struct RoundsHint {
    uint32_t rounds, slack;
};
inline RoundsHint nextRoundsHint(RoundsHint h, uint32_t ran, uint32_t needed) {
    if (ran > h.rounds) return RoundsHint{std::min(ran, kMaxRounds), 0};
    if (needed < h.rounds && ran == 0) return h.slack + 1 >= 4 ? RoundsHint{needed, 0} : RoundsHint{h.rounds, h.slack + 1};
    return RoundsHint{h.rounds, 0};
}
// do most of the slots in play pass the remainder screen?  -1: no slot in play, the history stays
inline int nextRemainderSeen(uint32_t inPlay, uint32_t survivors) { return !inPlay ? -1 : survivors * 4 >= inPlay * 3 ? 1 : 0; }

}  // namespace grokplan
