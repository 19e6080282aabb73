"""Test-only: Match lists and values for tests/test_gpu_grok_fused_round0.py -- the Grok plan's fused round 0 (csrc/grok_device.hip phase
2a: tdfa_wave_multi_kernel over the candidates of every entry whose round 0 walks tables in global memory, one grok_post_kernel launch
behind it).  An entry is a tag and the body of a chunk-edge family (tests/helpers/chunk_edges.py) with named groups; its values are
that family's cases with the tag in front, generated with the family's offset reduced by the tag's length, so that the event the kind
names still falls on W256_P of the TAGGED value.  The tag is the entry's required literal: a value is a candidate of one entry only,
and every job's rows show in the result.  Not part of the product."""
from collections import namedtuple

import numpy as np

from tests.helpers import chunk_edges as ce

TAG_BYTES = 4
BODIES = {   # family -> its pattern with named groups; {k} = the entry's number
    "log": r"(?P<a{k}>[^,]*),(?P<b{k}>\d*);(?P<c{k}>[^ ]*) (?P<d{k}>.*)",
    "big": r"(?P<a{k}>[^,]*),(?P<b{k}>\d*);(?:a|b)*a(?:a|b){{12}}(?P<c{k}>c+)(?P<d{k}>d*) (?P<e{k}>.*)",
    "lazy": r"(?P<a{k}>[^,]*),(?P<b{k}>\d*);(?:a|b)*a(?:a|b){{14}}(?P<c{k}>c+)(?P<d{k}>d*) (?P<e{k}>.*)",
    "over64": r"(?P<a{k}>[^;]*);(?P<b{k}>.*)a(?P<c{k}>.{{70}})",
    "over128": r"(?P<a{k}>[^;]*);(?P<b{k}>.*)a(?P<c{k}>.{{140}})",
    "quasi": r"Group = (?P<g{k}>.*), IP = (?P<ip{k}>\d+), NAT",
    "look": r"(?<![0-9.])(?P<o{k}>\d+)\.(?P<p{k}>\d+)\.(?P<q{k}>\d+)\.(?P<r{k}>\d+)(?![0-9])",
}
RUN_CAPTURE = r"^T{k:02d}:(?P<h{k}>[a-z]+) (?=(?P<m{k}>[^|]*))(?P<r{k}>[^ ]*) (?P<s{k}>.*)"      # (?=(S*)): a run capture, never in the fused launch
JUNK = b"xyz -"                                                                              # in front of the tag of a search entry
FILLER = b";7, "                                                                             # between the values of a packed batch
BORDER_COUNTS = (1, 3, 4, 5, 8, 9, 2, 7)                                                     # candidates per entry: full and ragged last workgroups of 4

Value = namedtuple("Value", "entry family kind variant p head bytes after")


def tag(k):
    return b"T%02d:" % k


def entry(k, family, anchored=True, tagged=True):
    return ("^" if anchored else "") + (tag(k).decode() if tagged else "") + BODIES[family].format(k=k)


def family_values(k, family, tagged=True, junk=False, training=False):
    """the cases of `family` for entry k, one per (kind, offset, variant), the residues 0..3 dealt round; the offset p is that of the
    event in the value as it is matched (tag included).  junk: every third value of a search entry has junk in front of its tag (the
    event moves by its length: p says where it is).  training: the lazy family's training lines instead (p = -1)"""
    fam = ce.FAMILIES[family]
    shift = TAG_BYTES if tagged else 0
    out = []
    if training:
        return [Value(k, family, "training", "", -1, i % 4, tag(k) + line, fam.after) for i, line in enumerate(fam.training())]
    i = 0
    for kind, min_p in fam.kinds.items():
        if kind == "resume":
            continue                                                                          # (a Grok entry's first search starts at 0)
        for P in ce.W256_P:
            if P - shift < min_p:
                continue
            for variant, line, after, frm in fam.cases(kind, P - shift):
                front = JUNK[:1 + i % len(JUNK)] if junk and i % 3 == 2 else b""
                out.append(Value(k, family, kind, variant, P + len(front), i % 4, front + (tag(k) if tagged else b"") + line, after or fam.after))
                i += 1
    return out


def run_capture_values(k, n=41):
    """values of the run-capture entry: the run [^|]* ends at a '|', or at the end of the value, at varying offsets"""
    out = []
    for i in range(n):
        run = ce._cyc(b"uv w", 1 + 7 * i % 300, i)
        line = tag(k) + b"host " + run.replace(b" ", b"_", 1)[:1] + run[1:] + (b"|rest" if i % 3 else b"")
        out.append(Value(k, "run", "run", "", len(line), i % 4, line, b"|"))
    return out


def pack(values, seed=20261019):
    """the values shuffled (seeded), each at its residue mod 4 of a 16-byte aligned buffer, filler between them, the `after` byte behind
    each and guard bytes at the end -> (values in batch order, data, off, len)"""
    order = np.random.default_rng(seed).permutation(len(values))
    values = [values[int(i)] for i in order]
    buf, off = bytearray(), []
    for i, v in enumerate(values):
        buf += ce._cyc(FILLER, (v.head - len(buf)) % 4, i)
        off.append(len(buf))
        buf += v.bytes + v.after
    data = np.frombuffer(bytes(buf) + b"\0" * ce.GUARD_BYTES, np.uint8)
    return values, data, np.array(off, np.uint32), np.array([len(v.bytes) for v in values], np.uint32)


def mixed_list():
    """-> (Match list, values, training values of the lazy entry).  Entries: log as a search (junk in front of some tags), big anchored,
    a run capture BETWEEN two fused entries, the lazy family, quasi and look untagged, and an entry nobody is a candidate of."""
    match = [entry(0, "log", anchored=False), entry(1, "big"), RUN_CAPTURE.format(k=2), entry(3, "lazy"),
             entry(4, "quasi", anchored=False, tagged=False), entry(5, "look", anchored=False, tagged=False), entry(6, "log")]
    values = (family_values(0, "log", junk=True) + family_values(1, "big") + run_capture_values(2) + family_values(3, "lazy") +
              family_values(4, "quasi", tagged=False) + family_values(5, "look", tagged=False))
    return match, values, family_values(3, "lazy", training=True)


def border_list(n_entries):
    """n_entries of the log body, entry k with BORDER_COUNTS[k % 8] candidates taken in turn from the tagged log cases (every 7th, so
    that kinds and offsets mix) -> (Match list, values)"""
    match = [entry(k, "log") for k in range(n_entries)]
    pool = family_values(0, "log")
    values, at = [], 0
    for k in range(n_entries):
        for _ in range(BORDER_COUNTS[k % len(BORDER_COUNTS)]):
            v = pool[at * 7 % len(pool)]
            values.append(v._replace(entry=k, bytes=tag(k) + v.bytes[TAG_BYTES:]))
            at += 1
    return match, values


def overflow_list():
    """-> (Match list, values): the overflow families (the 65th / 129th live thread on an offset of W256_P of the tagged value, and the
    `at_cap` controls), the log family, and an entry nobody is a candidate of.  Entries 0 and 1 are thread-list programs whose
    values walk the plan's own chain: first chance, overflow list, nfa_wide_kernel, nfa_decide_kernel"""
    match = [entry(0, "over64"), entry(1, "over128"), entry(2, "log"), entry(3, "over64")]
    return match, family_values(0, "over64") + family_values(1, "over128") + family_values(2, "log")


def needs_wide(v):
    """the value's thread list outgrows nfa_match_kernel's 64 threads (every over128 value does: its controls peak at 128)"""
    return v.family == "over128" or (v.family == "over64" and not v.variant.startswith("at_cap"))
