"""Test-only: result buffers with sentinels around them, for GPU tests that fence a kernel's result writes.  Four sentinel rows lie in
front of and behind the capture table and the status bytes; the capture table starts 0 to 3 dwords into a 16-byte aligned allocation
(so that a kernel's 16-byte copy of a row and its dword loop both get their turn).  read() asserts that every sentinel outside the
table is untouched and hands back the rows.  Not part of the product."""
GUARD = 4                      # sentinel rows in front of and behind the results
CAPS_SENTINEL, STATUS_SENTINEL = -7, 9


class GuardedResults:
    def __init__(self, torch, n, ngroups, caps_shift=0, status_fill=STATUS_SENTINEL):
        """room for n rows of 2 * ngroups capture offsets and n status bytes, everything filled with the sentinels; status_fill: what
        the status bytes, guards included, hold instead of their sentinel (a stale LC_OVERFLOW of an earlier launch, say)"""
        dev = torch.device("cuda:0")
        self.n, self.n_out, self.status_fill = n, 2 * ngroups, status_fill
        words = (n + 2 * GUARD) * self.n_out
        self.buf = torch.full((words + 8,), CAPS_SENTINEL, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.first = caps_shift + GUARD * self.n_out
        self.d_caps = self.buf[self.first:self.first + max(n * self.n_out, 1)]
        assert (self.d_caps.data_ptr() - self.buf.data_ptr()) == 4 * self.first and (4 * GUARD * self.n_out) % 16 == 0   # (shift 0: 16-byte aligned rows)
        self.sbuf = torch.full((n + 2 * 4 * GUARD,), status_fill, dtype=torch.uint8, device=dev)
        self.d_status = self.sbuf[4 * GUARD:4 * GUARD + n]

    def read(self, where):
        """-> (caps[n, 2 * ngroups], status[n]) after the launch has been synchronised; `where` names the launch in a failure"""
        n, n_out, first = self.n, self.n_out, self.first
        out, sout = self.buf.cpu().numpy(), self.sbuf.cpu().numpy()
        assert (out[:first] == CAPS_SENTINEL).all(), ("rows in front of the capture table were written", where)
        assert (out[first + n * n_out:] == CAPS_SENTINEL).all(), ("rows behind the capture table were written", where)
        assert (sout[:4 * GUARD] == self.status_fill).all() and (sout[4 * GUARD + n:] == self.status_fill).all(), ("status guard bytes were written", where)
        return out[first:first + n * n_out].reshape(n, n_out), sout[4 * GUARD:4 * GUARD + n]
