"""Plain models of phase 1 of the speculative Grok matcher (csrc/grok_device.hip grokPlanPhase1; kernels in grok_plan_kernel.hpp and
grok_kernel.hpp), written from include/lc_grok.h and the layout headers (grok_literal_layout.h, screen_kernel_layout.h):

    literal pass   bit p of a value's mask = "entry p has no literal, or the value contains the (at most 32) last bytes of it"
    screens        bit p is cleared where entry p has a screen and the yes/no DFA, walked over exactly the value's bytes, rejects
    counts         candidates per entry, values whose first candidate is the entry, who shadows whom

Nothing here knows about chunks, lanes, 16-byte loads or length order: that is the point.  tests/test_grok_plan_model.py ties the
models to the Aho-Corasick blob and to the regex oracle; tests/test_gpu_grok_plan.py compares the kernels with them bit for bit."""
import numpy as np

SC_NSTATES, SC_NCLASSES, SC_START, SC_SINK, SC_OFF_ACCEPT, SC_OFF_TABLE, SC_TOTAL_BYTES, SC_HEADER_WORDS = 1, 2, 3, 4, 5, 6, 7, 8
NO_SINK = 0xFFFFFFFF
PLAN_WORDS = 64 + 64 + 64 * 64      # perEntry[64] | firstOf[64] | shadowBy[64][64]


def indexed_literals(required):
    """what the index keeps of each entry's required literal: its last 32 bytes (b"" = the entry has none)"""
    return [bytes(l)[-32:] for l in required]


def always_bits(lits):
    """entries without a literal: their bit is set for every value.  A list with fewer than two literals has no index at all
    (grok_mask_fill_kernel): every entry is a candidate for every value."""
    if sum(1 for l in lits if l) < 2:
        return (1 << len(lits)) - 1
    return sum(1 << p for p, l in enumerate(lits) if not l)


def literal_mask(lits, always, v):
    m = always
    for p, l in enumerate(lits):
        if l and not (always >> p) & 1 and l in v:
            m |= 1 << p
    return m


class Screen:
    """a screen blob taken apart once (screen_kernel_layout.h)"""

    def __init__(self, blob):
        blob = np.asarray(blob, dtype=np.uint32)
        raw = blob.view(np.uint8)
        self.nstates, self.ncls, self.start, self.sink = (int(blob[i]) for i in (SC_NSTATES, SC_NCLASSES, SC_START, SC_SINK))
        self.cmap = bytes(raw[SC_HEADER_WORDS * 4:SC_HEADER_WORDS * 4 + 256])
        a, t = int(blob[SC_OFF_ACCEPT]), int(blob[SC_OFF_TABLE])
        self.accept = raw[a:a + self.nstates].tolist()
        self.table = raw[t:t + 2 * self.nstates * self.ncls].view(np.uint16).tolist()
        self.table_bytes = 2 * self.nstates * self.ncls
        self.stage_bytes = int(blob[SC_TOTAL_BYTES]) - a

    def step(self, state, byte):
        return self.table[state * self.ncls + self.cmap[byte]]

    def walk(self, v, state=None):
        """byte by byte from the start state; stops at the sink and at the dead state 0 -> the state it ends in"""
        state = self.start if state is None else state
        table, ncls, sink = self.table, self.ncls, self.sink
        if state == sink or state == 0:
            return state
        for c in bytes(v).translate(self.cmap):
            state = table[state * ncls + c]
            if state == sink or state == 0:
                break
        return state

    def passes(self, v):
        s = self.walk(v)
        return s == self.sink or (s != 0 and bool(self.accept[s]))


def screen_pass(blob, v):
    return (blob if isinstance(blob, Screen) else Screen(blob)).passes(v)


def stage2_mask(lits, always, screens, v):
    """screens: per entry a Screen or None.  Only bits the literal pass left are looked at (as on the device: a cleared bit stays clear)."""
    m = literal_mask(lits, always, v)
    for p, sc in enumerate(screens):
        if sc is not None and (m >> p) & 1 and not sc.passes(v):
            m &= ~(1 << p)
    return m


def plan_counts(masks, n_patterns):
    """-> uint32[PLAN_WORDS]: perEntry[p] = values with bit p; firstOf[p] = values whose lowest bit is p; shadowBy[p * 64 + f] = values
    with bit p whose lowest bit is the earlier entry f"""
    masks = np.asarray(masks, dtype=np.uint64)
    out = np.zeros(PLAN_WORDS, dtype=np.uint32)
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)   # [n][64]
    any_bit = bits.any(axis=1)
    lowest = np.where(any_bit, bits.argmax(axis=1), 64)
    for p in range(n_patterns):
        out[p] = bits[:, p].sum()
        out[64 + p] = (lowest == p).sum()
    for p in range(64):
        has = bits[:, p] & (lowest < p)
        if has.any():
            f, c = np.unique(lowest[has], return_counts=True)
            out[128 + p * 64 + f] = c
    return out
