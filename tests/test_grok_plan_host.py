"""The host planner of the speculative Grok batch (csrc/grok_plan_host.hpp) on the CPU: levels, the deal of entries to streams, which
entries join the fused round 0, the chains as step lists, the order the steps are queued in, and the history rules.
tests/native/grok_plan_check.cpp is built with AddressSanitizer and UBSan and run as a child process.  The expected answers are
written out here from the rules as the header's comments state them; nothing is computed by calling the planner."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# step kinds, list selectors, flags and counter words (grok_plan_host.hpp)
FINISH_SHADOWER, SECOND_OVERFLOW, POST, TICK, SEARCH_FIRST, SEARCH_SECOND_POST, SHADOWED_FIRST, SHADOWED_SECOND_POST, ROUND, REMAINDER = range(10)
NONE, LIST_A, LIST_B, UNANCHORED, OVERFLOW = range(5)
TICK_BEGIN, TICK_END, GATE = 1, 2, 4
CW_UNANCHORED, CW_ROUND0, CW_BOUND, CW_OVERFLOW, CW_REMAINDER, CW_FILTERED = 1, 2, 59, 61, 62, 63


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grok_plan") / "grok_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "loongcollector_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "grok_plan_check.cpp")])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-2000:]
        return r.stdout.decode().split("\n")[:-1]
    return run


def flat(rows):
    return [x for r in rows for x in r]


# ---------------------------------------------------------------------------------------------- levels
def levels(plan, entries, shadow=(), flat_knob=1):
    """entries: (p, cand, first, table_walk); shadow: (p, f, count)  -> levels in list order, entries of level > 0, p's of the sorted table"""
    out = plan("levels", flat_knob, len(entries), *flat(entries), *flat(shadow))
    second, table = out[1].split(":")
    return [int(x) for x in out[0].split()], int(second), [int(x) for x in table.split()]


def test_levels_half_of_the_candidates_shadowed_is_levelled_one_fewer_is_not(plan):
    quiet = [(0, 8, 8, 0), (1, 8, 8, 0)]
    assert levels(plan, quiet + [(2, 8, 4, 0)])[0] == [0, 0, 1]       # shadowed = cand - first = 4: 4 * 2 >= 8
    assert levels(plan, quiet + [(2, 8, 5, 0)])[0] == [0, 0, 0]       # shadowed 3


def test_levels_a_shadower_counts_from_a_quarter_of_the_candidates(plan):
    # entry 1 waits for entry 0 (level 1); entry 2 goes one level behind entry 1 only if entry 1 shadows 2 of its 8 candidates
    base = [(0, 4, 4, 0), (1, 4, 0, 0), (2, 8, 4, 0)]
    assert levels(plan, base, [(1, 0, 4), (2, 1, 2)])[0] == [0, 1, 2]
    assert levels(plan, base, [(1, 0, 4), (2, 1, 1)])[0] == [0, 1, 1]


def test_levels_a_table_walk_entry_stays_at_level_0_unless_the_knob_is_off(plan):
    base = [(0, 4, 4, 0), (1, 4, 0, 0), (2, 8, 4, 1)]
    shadow = [(1, 0, 4), (2, 1, 2)]
    assert levels(plan, base, shadow)[0] == [0, 1, 0]
    assert levels(plan, base, shadow, flat_knob=0)[0] == [0, 1, 2]


def test_levels_a_chain_of_five_stops_at_level_3(plan):
    entries = [(0, 4, 4, 0)] + [(p, 4, 0, 0) for p in range(1, 5)]
    shadow = [(p, p - 1, 4) for p in range(1, 5)]
    assert levels(plan, entries, shadow) == ([0, 1, 2, 3, 3], 4, [0, 1, 2, 3, 4])


def test_levels_the_sorted_table_keeps_list_order_inside_a_level(plan):
    entries = [(0, 4, 4, 0), (3, 4, 0, 0), (5, 4, 4, 0), (7, 4, 0, 0), (9, 4, 4, 0)]
    assert levels(plan, entries, [(3, 0, 4), (7, 0, 4)]) == ([0, 1, 0, 1, 0], 2, [0, 5, 9, 3, 7])


# ---------------------------------------------------------------------------------------------- deal
def deal(plan, used, leftovers, entries):
    """entries: (cost, cost0, cost1, level, busy)  -> order, streams (-1: not dealt)"""
    out = plan("deal", used, leftovers, len(entries), *flat(entries))
    return [int(x) for x in out[0].split()], [int(x) for x in out[1].split()]


def test_deal_longest_first_to_the_least_loaded_stream_ties_in_index_order(plan):
    # loads: 20005 | 20005, then the 3 to stream 0 (the first of two equal loads), then the 1 to stream 1
    assert deal(plan, 2, 0, [(0, c, 0, 0, 0) for c in (5, 5, 3, 1)]) == ([0, 1, 2, 3], [0, 1, 0, 1])
    # one long entry keeps its stream to itself: 110000 | 30000 -> 60000 -> 90000
    assert deal(plan, 2, 0, [(0, c, 0, 0, 0) for c in (90000, 10000, 10000, 10000)]) == ([0, 1, 2, 3], [0, 1, 1, 1])
    assert deal(plan, 2, 0, [(0, c, 0, 0, 0) for c in (1, 3, 5, 5)]) == ([2, 3, 1, 0], [1, 0, 0, 1])


def test_deal_on_one_stream(plan):
    assert deal(plan, 1, 0, [(0, c, 0, 0, 0) for c in (5, 5, 3, 1)]) == ([0, 1, 2, 3], [0, 0, 0, 0])


def test_deal_an_unmeasured_entry_counts_fifty_times_its_estimate(plan):
    # 1000 * 50 = 50000 lies between the measured 40000 and 60000
    assert deal(plan, 3, 0, [(1000, 0, 0, 0, 0), (1, 40000, 0, 0, 0), (1, 60000, 0, 0, 0)]) == ([2, 0, 1], [1, 2, 0])
    # ... and the leftovers deal reads cost1, not cost0
    assert deal(plan, 3, 1, [(1000, 9, 0, 0, 1), (1, 9, 40000, 0, 1), (1, 9, 60000, 0, 1)])[0] == [2, 0, 1]


def test_deal_leftovers_skip_idle_entries_and_levels_from_2_on_round_0_skips_every_level_but_0(plan):
    entries = [(0, 0, 400000, 0, 1), (0, 0, 300000, 0, 0), (0, 0, 200000, 2, 1), (0, 0, 100000, 1, 1)]
    assert deal(plan, 2, 1, entries) == ([0, 1, 2, 3], [0, -1, -1, 1])
    assert deal(plan, 2, 0, [(0, 4, 0, 0, 0), (0, 3, 0, 1, 0), (0, 2, 0, 2, 0), (0, 1, 0, 0, 0)]) == ([0, 1, 2, 3], [0, -1, -1, 1])


# ---------------------------------------------------------------------------------------------- round 0
def fused(plan, wide_first, max_jobs, entries):
    """entries: (level, cand, first_nfa, prepare: 0 no / 1 yes / 2 stop)"""
    out = plan("fused", wide_first, max_jobs, len(entries), *flat(entries))[0]
    return out if out == "stop" else [int(x) for x in out.split()]


def test_fused_round_0_takes_the_level_0_entries_the_predicate_accepts(plan):
    entries = [(0, 5, 0, 1), (1, 5, 0, 1), (0, 5, 0, 0), (0, 5, 1, 1), (0, 5, 0, 1)]
    assert fused(plan, 1, 64, entries) == [1, 0, 0, 1, 1]
    assert fused(plan, 2, 64, entries) == [1, 0, 0, 0, 1]      # the knob forces the wide kernel on thread-list entries
    assert fused(plan, 1, 2, entries) == [1, 0, 0, 1, 0]       # the job table is full
    assert fused(plan, 1, 64, entries[:2] + [(0, 5, 0, 2)]) == "stop"


def test_early_rounds_by_the_entrys_history(plan):
    # (rounds, re is a TDFA, remainder seen)
    entries = [(2, 1, 1), (2, 1, 0), (2, 0, 1)]
    assert plan("early", 1, 0, len(entries), *flat(entries)) == [" 1 0 0"]
    assert plan("early", 1, 1, len(entries), *flat(entries)) == [" 0 0 0"]       # a calibration batch screens every entry
    assert plan("early", 2, 1, len(entries), *flat(entries)) == [" 1 1 0"]       # forced: every tagged DFA
    assert plan("early", 0, 0, len(entries), *flat(entries)) == [" 0 0 0"]


# ---------------------------------------------------------------------------------------------- chains
def step(kind, entry, arg=0, lst=NONE, out=NONE, count=0, flags=0):
    return "%d.%d.%d.%d.%d.%d.%d" % (kind, entry, arg, lst, out, count, flags)


def second_overflow(a):
    return [step(SECOND_OVERFLOW, a, 0, OVERFLOW, NONE, CW_OVERFLOW, TICK_BEGIN), step(POST, a, 0, OVERFLOW, NONE, CW_OVERFLOW)]


def search_proper(a):
    return [step(SEARCH_FIRST, a, 0, UNANCHORED, LIST_B, CW_UNANCHORED), step(SEARCH_SECOND_POST, a, 0, LIST_B, NONE, CW_FILTERED)]


def shadowed(a):
    return [step(SHADOWED_FIRST, a, 0, NONE, OVERFLOW, CW_OVERFLOW, TICK_BEGIN), step(SHADOWED_SECOND_POST, a, 0, OVERFLOW, NONE, CW_OVERFLOW)]


def tick(a, which):
    return [step(TICK, a, flags=which)]


def remainder(a):
    return [step(REMAINDER, a)]


def chains(plan, used, entries, shadow=()):
    """entries: (p, level, cand, rounds, anchored, early, cost1, ov, un, round0, bound)
    -> step lists per owner, early mask, covered mask, (busy, stream, owner, queued) per entry"""
    out = plan("chains", used, len(entries), *flat(entries), *flat(shadow))
    n = len(entries)
    lists = [line.split(":")[1].split() for line in out[:n]]
    masks = out[n].split()
    per = [tuple(int(x) for x in e.split(",")) for e in out[n + 1].split()]
    return lists, int(masks[1]), int(masks[3]), per


def one(plan, anchored=0, early=0, ov=0, un=0, round0=0, rounds=3):
    lists, early_mask, covered, per = chains(plan, 1, [(0, 0, 10, rounds, anchored, early, 0, ov, un, round0, 0)])
    return lists[0], early_mask, covered, per[0]


def test_chain_of_a_level_0_entry_with_overflowed_slots_only(plan):
    assert one(plan, ov=3, round0=4) == (second_overflow(0) + tick(0, TICK_END) + remainder(0), 0, 1, (1, 0, 0, 0))
    assert one(plan, anchored=1, ov=3)[0] == second_overflow(0) + tick(0, TICK_END) + remainder(0)   # (nothing unanchored: no search proper)


def test_chain_with_unanchored_slots_runs_the_search_proper_between(plan):
    want = second_overflow(0) + search_proper(0) + tick(0, TICK_END) + remainder(0)
    assert one(plan, anchored=1, ov=3, un=2) == (want, 0, 1, (1, 0, 0, 0))


def test_chain_with_unanchored_slots_and_no_overflow_begins_with_a_bare_tick(plan):
    want = tick(0, TICK_BEGIN) + search_proper(0) + tick(0, TICK_END) + remainder(0)
    assert one(plan, anchored=1, un=2) == (want, 0, 1, (1, 0, 0, 0))


def test_an_entry_with_nothing_but_slots_in_play_has_no_steps_and_is_covered(plan):
    assert one(plan, round0=5) == ([], 0, 1, (0, -1, 0, 0))     # (its screens went out ahead of the counts)
    assert one(plan) == ([], 0, 0, (0, -1, 0, 0))


def test_a_level_1_entry_whose_values_are_all_won_queues_nothing(plan):
    quiet = (0, 0, 10, 3, 0, 0, 0, 0, 0, 0, 0)
    lists, _, covered, per = chains(plan, 2, [quiet, (1, 1, 10, 3, 1, 0, 0, 0, 0, 0, 0)])
    assert lists == [[], []] and covered == 0 and per[1] == (0, -1, 1, 0)
    lists, _, covered, per = chains(plan, 2, [quiet, (1, 1, 10, 3, 1, 0, 0, 0, 0, 0, 4)])
    assert lists == [[], shadowed(1) + search_proper(1) + tick(1, TICK_END) + remainder(1)] and covered == 2 and per[1] == (1, 0, 1, 0)
    lists = chains(plan, 2, [quiet, (1, 1, 10, 3, 0, 0, 0, 0, 0, 0, 4)])[0]
    assert lists[1] == shadowed(1) + tick(1, TICK_END) + remainder(1)                  # (no anchored search: no search proper)


def test_a_level_2_entry_rides_behind_its_main_shadower(plan):
    entries = [(0, 0, 10, 3, 0, 0, 300000, 1, 0, 0, 0),
               (1, 1, 10, 3, 0, 0, 200000, 0, 0, 0, 5),
               (2, 1, 10, 3, 0, 0, 100000, 0, 0, 0, 5),
               (3, 2, 10, 3, 0, 0, 900000, 0, 0, 0, 5),
               (4, 3, 10, 3, 0, 0, 900000, 0, 0, 0, 5)]
    # entry 3's main shadower is the largest shadow[3][f] among ACTIVE f: list entry 5 is not in the batch
    shadow = [(3, 1, 2), (3, 2, 6), (3, 5, 50), (4, 3, 9)]
    lists, early, covered, per = chains(plan, 3, entries, shadow)
    own = shadowed(2) + tick(2, TICK_END) + remainder(2)
    ride3 = [step(FINISH_SHADOWER, 3, 2)] + shadowed(3) + tick(3, TICK_END) + remainder(3)
    ride4 = [step(FINISH_SHADOWER, 4, 3)] + shadowed(4) + tick(4, TICK_END) + remainder(4)
    assert lists[0] == second_overflow(0) + tick(0, TICK_END) + remainder(0)
    assert lists[1] == shadowed(1) + tick(1, TICK_END) + remainder(1)
    assert lists[2] == own + ride3 + ride4 and lists[3] == [] and lists[4] == []
    # streams: the leftovers deal gives 0, 1, 2 to entries 0, 1, 2 (dearest first); 3 and 4 take their shadower's
    assert per == [(1, 0, 0, 0), (1, 1, 1, 0), (1, 2, 2, 0), (1, 2, 2, 0), (1, 2, 2, 0)]
    assert (early, covered) == (0, 31)


def test_an_early_entry_gets_its_rounds_unscreened_and_no_remainder_step(plan):
    want = [step(ROUND, 0, 1, LIST_A, LIST_B, CW_ROUND0), step(ROUND, 0, 2, LIST_B, LIST_A, CW_ROUND0 + 1),
            step(ROUND, 0, 3, LIST_A, LIST_B, CW_ROUND0 + 2, GATE)]
    assert one(plan, early=1, rounds=4) == (want, 1, 0, (0, -1, 0, 1))        # (not busy: it keeps the stream round 0 gave it)
    lists, early, covered, per = one(plan, early=1, ov=2, rounds=2)
    assert lists == second_overflow(0) + tick(0, TICK_END) + [step(ROUND, 0, 1, LIST_A, LIST_B, CW_ROUND0, GATE)]
    assert (early, covered, per) == (1, 0, (1, 0, 0, 1))


def test_round_r_reads_and_writes_the_lists_in_turn(plan):
    # screened: round 1 reads the survivors of the remainder screen (on the unanchored list, counted in GC_REMAINDER)
    assert plan("rounds", 5, 4, 1)[0].split() == [step(ROUND, 5, 1, UNANCHORED, LIST_B, CW_REMAINDER), step(ROUND, 5, 2, LIST_B, LIST_A, CW_ROUND0 + 1),
                                                  step(ROUND, 5, 3, LIST_A, LIST_B, CW_ROUND0 + 2, GATE)]
    assert plan("rounds", 5, 4, 0)[0].split() == [step(ROUND, 5, 1, LIST_A, LIST_B, CW_ROUND0), step(ROUND, 5, 2, LIST_B, LIST_A, CW_ROUND0 + 1),
                                                  step(ROUND, 5, 3, LIST_A, LIST_B, CW_ROUND0 + 2, GATE)]
    assert plan("rounds", 5, 2, 1)[0].split() == [step(ROUND, 5, 1, UNANCHORED, LIST_B, CW_REMAINDER, GATE)]


# ---------------------------------------------------------------------------------------------- queue order
def test_queue_order_is_step_k_of_every_chain_before_step_k_plus_1(plan):
    assert plan("queue", 3, 3, 1, 2, 2, 0, 1)[0].split() == ["2.0", "0.0", "1.0", "2.1", "0.1", "0.2"]
    assert plan("queue", 3, 3, 1, 2, 0, 1, 2)[0].split() == ["0.0", "1.0", "2.0", "0.1", "2.1", "0.2"]
    assert plan("queue", 2, 0, 0, 0, 1) == [""]


# ---------------------------------------------------------------------------------------------- history
def test_history_a_batch_that_ran_more_rounds_raises_the_hint_and_clears_the_slack(plan):
    assert plan("hint", 3, 2, 5, 1) == ["5 0"]
    assert plan("hint", 3, 2, 100, 1) == ["56 0"]      # GC_BOUND - GC_ROUND0 - 1 rounds can be queued ahead
    assert plan("hint", 3, 2, 3, 1) == ["3 0"]         # (ran as many as the hint: nothing to learn, the slack starts again)


def test_history_four_batches_in_a_row_that_needed_fewer_rounds_lower_the_hint(plan):
    assert plan("hint", 3, 0, 0, 2) == ["3 1"]
    assert plan("hint", 3, 1, 0, 2) == ["3 2"]
    assert plan("hint", 3, 2, 0, 2) == ["3 3"]
    assert plan("hint", 3, 3, 0, 2) == ["2 0"]
    assert plan("hint", 3, 3, 0, 3) == ["3 0"]         # a batch that needed them all in between: from the start


def test_history_rounds_needed_is_one_past_the_last_round_that_left_values_in_play(plan):
    assert plan("needed", 4, 0, 5, 0, 2, 9) == ["4"]   # (rounds - 1 words are looked at: the 9 is not)
    assert plan("needed", 4, 0, 5, 0, 0, 9) == ["2"]
    assert plan("needed", 4, 0, 0, 0, 0, 0) == ["1"]
    assert plan("needed", 4, 7, 5, 5, 5, 5) == ["1"]   # (the entry went on behind its queued rounds: `ran` speaks)


def test_history_the_wide_word_sets_8_and_an_idle_batch_counts_it_down(plan):
    assert plan("overflow", 0, 1) == ["8"] and plan("overflow", 3, 1) == ["8"]
    assert plan("overflow", 8, 0) == ["7"] and plan("overflow", 1, 0) == ["0"] and plan("overflow", 0, 0) == ["0"]


def test_history_survivors_from_three_quarters_of_the_slots_in_play_set_remainder_seen(plan):
    assert plan("remainder", 8, 6) == ["1"] and plan("remainder", 8, 5) == ["0"] and plan("remainder", 4, 3) == ["1"]
    assert plan("remainder", 0, 0) == ["-1"]           # no slot in play: the history stays
