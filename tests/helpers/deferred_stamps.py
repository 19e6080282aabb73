"""Test-only restatement of the DEFERRED-STAMP walk of the one-stamp pair kernel (csrc/tdfa_stream_kernel.hpp
tdfaStreamPair1Chunk with kLabDeferStamps, tdfaDeferPush / tdfaDeferFlush), store for store.

What is different from TdfaPair1Interp (tests/helpers/table_interp.py): a pair's stamp is not written when the pair is stepped.
A lane turns it into an EVENT (register index, +1 flag, position) and, if the register is a real one, pushes it onto a queue
of two (e1 = e0; e0 = event).  The WAVE flushes -- every lane writes e1, then e0, empty slots into the dummy row, then both
slots are emptied -- as soon as some lane holds two events; before the second registers of a chunk's DOUBLE entries are settled,
when some lane of the wave met one in that chunk; and at the end of the line.  The flush is a decision of the whole wave, so
the walk is of up to 64 lines in lockstep: a lane whose line has ended goes on stepping the identity column, as in the kernel.

Not part of the product, never imported by loongcollector_amd/.
"""
from tests.helpers.table_interp import TdfaPair1Interp, _with_run_captures

QUEUE_DEPTH = 2


class DeferredPair1Wave(TdfaPair1Interp):
    def __init__(self, rx, compact=True):
        super().__init__(rx, compact=compact)
        self.stores = 0          # register stores issued per lane by the last walk (flush slots + settled doubles)
        self.flushes = 0         # flushes of the last walk (the one at the end of the line included)
        self.max_real_in_chunk = 0   # most real stamps one lane met in one chunk
        self.double_flushes = 0  # flushes in front of a settle that found an event of the settled register pending

    def walk_wave(self, lines, head=0, chunk=8):
        """-> one result per line (flat caps or None), as fullmatch_pair1 gives them"""
        assert 1 <= len(lines) <= 64
        mask = 0xFFFF if self.compact else 0xFFFFFFFF
        dummy = self.nregs - 1
        n = len(lines)
        regs = [[0] * self.nregs for _ in range(n)]
        row0 = self.p_base + (self.start_row - 320) // self.row_bytes * self.p_row
        rows = [row0] * n
        totals = [head + len(s) if s else 0 for s in lines]
        queue = [[] for _ in range(n)]                       # oldest first; at most QUEUE_DEPTH events (ra, value)
        self.stores = self.flushes = self.max_real_in_chunk = self.double_flushes = 0

        def flush():
            for lane in range(n):                            # e1 then e0: first in, first out; empty slots write the dummy row
                for ra, val in queue[lane]:
                    regs[lane][ra] = val
                del queue[lane][:]
            self.stores += QUEUE_DEPTH
            self.flushes += 1

        m = 0
        while m * chunk < max(totals):
            pending = [[] for _ in range(n)]                 # DOUBLE entries of this chunk per lane: (rB, value)
            real = [0] * n
            for p in range(chunk // 2):
                i0 = m * chunk + 2 * p
                for lane, s in enumerate(lines):
                    inside0, inside1 = head <= i0 < totals[lane], head <= i0 + 1 < totals[lane]
                    ca = int(self.cmapa[s[i0 - head]]) if inside0 else self.p_ida
                    cb = int(self.cmap[s[i0 + 1 - head]]) if inside1 else self.id_col
                    e = int(self.blob[(rows[lane] + ca + cb) // 4])
                    rows[lane] = e & 0xFFFF
                    pbase = i0 - head
                    ra, delta = (e >> 16) & 0x7F, (e >> 23) & 1
                    if ra != dummy:                          # the push: real events only
                        assert 0 <= pbase + delta < len(s)
                        assert len(queue[lane]) < QUEUE_DEPTH
                        queue[lane].append((ra, (pbase + delta) & mask))
                        real[lane] += 1
                    if e >> 31:
                        pending[lane].append(((e >> 24) & 0x7F, (pbase + 1) & mask))
                if any(len(q) == QUEUE_DEPTH for q in queue):    # the wave's decision, behind every pair
                    flush()
            self.max_real_in_chunk = max(self.max_real_in_chunk, max(real))
            if any(pending):                                 # some lane met a DOUBLE: the queue goes first (see the kernel's comment)
                if any(rb == ra for lane in range(n) for rb, _ in pending[lane] for ra, _ in queue[lane]):
                    self.double_flushes += 1
                flush()
                for lane in range(n):
                    for rb, val in pending[lane]:
                        regs[lane][rb] = max(regs[lane][rb], val)
                        self.doubles += 1
                self.stores += chunk // 2
            m += 1
        flush()                                              # the end of the line: nothing stays behind
        assert not any(queue)
        out = []
        for lane, s in enumerate(lines):
            r = regs[lane]
            for w in self.fold or ():
                for k in (1, 2, 3):
                    x = (w >> (8 * k)) & 0xFF
                    if x != 0xFF:
                        r[x] = max(r[x], r[w & 0xFF])
            for b, a, delta in self.derive:
                r[b] = (r[a] + delta) & mask
            state = (rows[lane] - self.p_base) // self.p_row
            fid = int(self.final_id[state])
            if state == 0 or fid == 0xFFFF:
                out.append(None)
                continue
            caps = []
            for sl in range(self.nslots):
                mm = int(self.final_map[fid * self.nslots + sl])
                caps.append(len(s) if mm == 0xFF else -1 if mm == 0xFE else r[mm])
            out.append(self._runs(s, caps))
        return out

    def _runs(self, s, caps):
        return _with_run_captures(lambda self_, s_: caps)(self, s)
