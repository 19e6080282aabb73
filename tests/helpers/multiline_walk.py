"""The multiline processors' record walk on FLAG BYTES, as ONE sequential pass over the items: no slices, no summaries, no queue.  The
reference the record scan (csrc/multiline_scan.hpp, ml_flags_kernel / ml_bounds_kernel of csrc/multiline_kernel.hpp) is held against
at sizes and shapes that real lines and regexes do not reach.

What is restated, from the reference's line numbers and not from multiline_scan.hpp:
  ProcessorSplitMultilineLogStringNative::ProcessEvent (core/plugin/processor/inner/ProcessorSplitMultilineLogStringNative.cpp:161-298),
  HandleUnmatchLogs (:341-380), and -- with off=None -- ProcessorMergeMultilineLogNative::MergeLogsByRegex (:161-330), which walks
  events with the same automaton and hands whole events to its HandleUnmatchLogs (:360-392).
The per-item questions "does it match the start / continue / end pattern" are bits 0, 1, 2 of the item's flag byte; bit 3 says, for lines
of a read buffer, that the line is empty.  A bit of a pattern that the mode does not use is never read.

Three rules of the walk that are easy to lose:
  * HandleUnmatchLogs' loop `while (begin < sourceVal.size())` (:350) ends BEFORE an empty last line of the range it is handed: that
    line is neither emitted nor counted (_unmatched_last);
  * the flush (:288-298) hands over [multiStart, size): an empty last line there still has its line feed behind it and is kept;
  * "end alone" enters with isPartialLog = true and multiStart = 0 (:161-165).
Two rules of the record writers (csrc/multiline_kernel.hpp MlDeviceWriter, csrc/multiline_gpu.cpp MlHostWriter):
  * LC_ML_LAST is set when the emitter is the flush, or the emitter is the last item of a value without a trailing separator
    (off[n] == nbytes + 1): isLastLog of :174 (_last_bit);
  * the flush's matched record runs to nbytes (:290-292: the rest of the source value, a trailing line feed included).

tests/test_multiline_walk.py holds this walk against MultilineOracle.split (real lines, real regexes) through flags_and_table() below;
that comparison is what makes it a reference.  The two rule functions are module attributes so that the mutation checks there can
replace them."""
from loongcollector_amd import multiline as ML

F_START, F_CONT, F_END, F_EMPTY = 1, 2, 4, 8
REC_MATCHED, REC_RUN, REC_LAST = 1, ML.ML_RUN, ML.ML_LAST
# counts of walk(): the six words of the library's counts[] that the scan itself decides
CNT_NAMES = ("items", "unmatched", "matched_logs", "records", "final_partial", "final_start")
CNT_WORDS = (0, 1, 2, 3, 6, 7)          # their places in counts[LC_ML_CNT_WORDS] (4, 5: LC_OVERFLOW / LC_GAVE_UP answers, ml_flags_kernel's)


def _unmatched_last(flags, last, from_flush):
    """the last item HandleUnmatchLogs emits of a range that ends with item `last` (:350)"""
    if not from_flush and flags[last] & F_EMPTY:
        return last - 1
    return last


def _last_bit(emitter, n, tail_unterminated):
    """isLastLog of the emission (:174, :288-298)"""
    return REC_LAST if (emitter >= n or (tail_unterminated and emitter == n - 1)) else 0


def walk(mode, flags, off=None, nbytes=0):
    """-> (records [(begin, length, flag word)], counts (items, unmatched, matched logs, records, final partial, final start))"""
    has_start, has_cont, has_end = bool(mode & ML.ML_HAS_START), bool(mode & ML.ML_HAS_CONT), bool(mode & ML.ML_HAS_END)
    discard, flush = bool(mode & ML.ML_DISCARD), bool(mode & ML.ML_FLUSH)
    flags = flags.tolist() if hasattr(flags, "tolist") else [int(f) for f in flags]
    n = len(flags)
    if off is None:
        flags = [f & 7 for f in flags]      # (events have no "empty last line" rule)
    else:
        off = off.tolist() if hasattr(off, "tolist") else [int(x) for x in off]
    tail_unterminated = off is not None and n > 0 and off[n] == nbytes + 1
    out = []
    unmatched_items = matched_logs = 0

    def matched(first, last, emitter):
        nonlocal matched_logs
        matched_logs += 1
        fl = REC_MATCHED | _last_bit(emitter, n, tail_unterminated)
        if off is None:
            out.append((first, last - first + 1, fl))
        else:
            b = off[first]
            out.append((b, nbytes - b if emitter >= n else off[last + 1] - 1 - b, fl))

    def unmatched(first, last, emitter):
        nonlocal unmatched_items
        last = _unmatched_last(flags, last, emitter >= n)
        if last < first:
            return
        unmatched_items += last - first + 1
        if discard:
            return
        fl = _last_bit(emitter, n, tail_unterminated)
        if off is None:
            out.append((first, 1, fl))
            out.extend((k, 1, fl | REC_RUN) for k in range(first + 1, last + 1))
        else:
            out.append((off[first], off[first + 1] - 1 - off[first], fl))
            out.extend((off[k], off[k + 1] - 1 - off[k], fl | REC_RUN) for k in range(first + 1, last + 1))

    partial = (not has_start) and (not has_cont) and has_end        # :161-165
    ms = 0
    for i, f in enumerate(flags):
        if not partial:
            if f & (F_START if has_start else F_CONT):               # :176-184
                ms, partial = i, True
            elif has_end and not has_start and has_cont and f & F_END:  # continue + end, :187-192
                matched(i, i, i)
            else:
                unmatched(i, i, i)
            continue
        if has_cont and f & F_CONT:                                  # :199-203
            continue
        if has_end:
            if has_cont:                                             # :206-228
                if f & F_END:
                    matched(ms, i, i)
                else:
                    unmatched(ms, i, i)
                partial = False
            elif f & F_END:                                          # start + end, or end alone, :229-246
                matched(ms, i, i)
                if has_start:
                    partial = False
                else:
                    ms = i + 1
        elif not has_cont:                                           # start alone, :250-260
            if f & F_START:
                matched(ms, i - 1, i)
                ms = i
        else:                                                        # start + continue, :261-282
            matched(ms, i - 1, i)
            if f & F_START:
                ms = i
            else:
                unmatched(i, i, i)
                partial = False
    if flush and partial and ms < n:                                 # :288-298
        if not has_end:
            matched(ms, n - 1, n)
        else:
            unmatched(ms, n - 1, n)
    return out, (n, unmatched_items, matched_logs, len(out), int(partial), ms)


def counts_of_library(counts8):
    """the walk's six counters out of a counts[LC_ML_CNT_WORDS] of the library"""
    return tuple(int(counts8[w]) for w in CNT_WORDS)


# ---------------------------------------------------------------------------------------------- real lines -> flag bytes
SCAN_CONFIGS = [
    {"StartPattern": r"\d{4}-\d{2}-\d{2} .*"},
    {"StartPattern": r"\[\w+\]", "ContinuePattern": r"\s+at\s.*", "UnmatchedContentTreatment": "discard"},
    {"StartPattern": r"\[\w+\]", "ContinuePattern": r"\s+at\s.*"},
    {"StartPattern": "BEGIN", "EndPattern": r"END\d*$"},
    {"StartPattern": "BEGIN", "EndPattern": r"END\d*$", "UnmatchedContentTreatment": "discard"},
    {"ContinuePattern": r"\s+.*", "EndPattern": r"\}"},
    {"ContinuePattern": r"\s+.*", "EndPattern": r"\}", "UnmatchedContentTreatment": "discard"},
    {"EndPattern": ";$", "UnmatchedContentTreatment": "discard"},
    {"EndPattern": ";$"},
    {"StartPattern": r"\[\w+\].*", "ContinuePattern": r"\s+at\s.*", "EndPattern": r"\}$"},
    {"StartPattern": ".*"},
]
POOL = [b"2024-01-04 boom", b"  at com.example.A.b(A.java:1)", b"[ERROR] x", b"BEGIN tx", b"END7", b"END", b"END7x", b"}x", b"}", b"{",
        b"stmt;", b"noise", b"", b"\tcontinued", b"2024-13-99 not checked"]
BIASES = (None, 1, 11, 13, 12)          # some buffers are dominated by one kind of line


def biased_buffer(rng, n, bias):
    """n lines of POOL, nine in ten of them POOL[bias] when a bias is given; three in ten buffers end with a line feed"""
    val = b"\n".join(POOL[bias] if bias is not None and rng.random() < 0.9 else rng.choice(POOL) for _ in range(n))
    if rng.random() < 0.3:
        val += b"\n"
    return val


def flags_and_table(o, val):
    """what the device computes before the scan: the split kernels' line table and the three answers per line (here: the oracle's
    regexes, line by line)"""
    lines = val.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()          # a trailing line feed does not open an empty last line (GetNextLine :382-392)
    off, at = [], 0
    for ln in lines:
        off.append(at)
        at += len(ln) + 1
    off.append(at)           # len[i] = off[i+1] - off[i] - 1, also for an unterminated last line
    hit = lambda rx, ln: 1 if (rx is not None and rx.prefixmatch(ln) is not None) else 0
    flags = [hit(o.start, ln) | hit(o.cont, ln) << 1 | hit(o.end, ln) << 2 | (8 if not ln else 0) for ln in lines]
    mode = (ML.ML_HAS_START if o.start else 0) | (ML.ML_HAS_CONT if o.cont else 0) | (ML.ML_HAS_END if o.end else 0) | \
        (ML.ML_DISCARD if o.discard else 0) | ML.ML_FLUSH
    return mode, flags, off
