"""lc_grok_match_device on a resident batch, for the GPU Grok tests."""
import numpy as np


def device_rows(torch, g, values, extra_cap=None, packed=None, scratch_fill=None, d_scratch=None):
    """lc_grok_match_device on a resident batch -> (pattern, first, extra sorted by (line, seq), stats).  packed: a ready-made
    (data, off, len) in the place of `values` -- the values keep the residues their offsets give them (the device copy is 16-byte
    aligned); scratch_fill: the byte the scratch area is filled with (default: whatever the allocation holds); d_scratch: the caller's
    scratch area, as the last batch left it"""
    dev = torch.device("cuda:0")
    if packed is None:
        n = len(values)
        data = np.frombuffer(b"".join(values) + b"\0" * 16, dtype=np.uint8)
        length = np.array([len(v) for v in values], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint32)
        off[1:] = np.cumsum(length[:-1], dtype=np.uint64).astype(np.uint32)
    else:
        data, off, length = (np.ascontiguousarray(a, dtype=t) for a, t in zip(packed, (np.uint8, np.uint32, np.uint32)))
        n = len(off)
        assert len(length) == n and (n == 0 or int((off.astype(np.int64) + length).max()) + 16 <= len(data))
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    d_len = torch.from_numpy(length.view(np.int32).copy()).to(dev)
    row = g.row_ints
    d_pattern = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty((n, row), dtype=torch.int32, device=dev)
    d_extra = torch.empty((extra_cap if extra_cap is not None else 6 * n + 1024, row + 2), dtype=torch.int32, device=dev)
    d_nextra = torch.zeros(1, dtype=torch.int32, device=dev)
    if d_scratch is None:
        d_scratch = torch.empty(g.scratch_bytes(n), dtype=torch.uint8, device=dev)
    assert d_scratch.numel() >= g.scratch_bytes(n)
    assert packed is None or d_data.data_ptr() % 16 == 0
    if scratch_fill is not None:
        d_scratch.fill_(scratch_fill)
    try:
        g.match_device(d_data, d_off, d_len, n, d_pattern, d_first, d_extra, d_nextra, d_scratch)
    except RuntimeError:
        # LC_ERR_OVERFLOW: d_nextra says how many rows are needed (the speculative path keeps the further matches of EVERY candidate
        # entry until the winner is known, so its temporary rows can run out where the final rows would have fitted)
        need = int(d_nextra.cpu()[0])
        assert need > d_extra.shape[0]
        d_extra = torch.empty((need, row + 2), dtype=torch.int32, device=dev)
        g.match_device(d_data, d_off, d_len, n, d_pattern, d_first, d_extra, d_nextra, d_scratch)
    stats = g.last_batch_stats()
    nx = int(d_nextra.cpu()[0])
    extra = d_extra[:nx].cpu().numpy()
    if nx:
        extra = extra[np.lexsort((extra[:, 1], extra[:, 0]))]
    pattern, first = d_pattern.cpu().numpy(), d_first.cpu().numpy()
    first[pattern < 0] = -1   # (rows of values nobody won are unspecified on the sequential path)
    return pattern, first, extra, stats
