"""processor_parse_apsara_gpu on the device: apsara_parse_kernel over every fixture line through lc_apsara_parse_device and
lc_apsara_parse_host against the per-line routine compiled for the host, the processor over every fixture group against the recorded
output of the reference's own processor, the edges of the stage walk at the smallest shapes that can break, sentinel-guarded outputs,
and 64 Ki seeded random lines."""
import os
import random

import numpy as np
import pytest

from helpers import apsara_double as ad

pytestmark = pytest.mark.gpu
SENT = -7
D = b"[2013-03-13 18:05:09.493309]"


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fixtures():
    return ad.load_fixtures()


@pytest.fixture(scope="module")
def fixture_lines(fixtures):
    """every source value of both fixture files (the unit test's multi-line values among them)"""
    return ad.all_lines(*fixtures)


_HOST = {}


def host_rows(lines, W):
    """the per-line routine on the host, once per (line, W)"""
    out = []
    for ln in lines:
        key = (ln, W)
        if key not in _HOST:
            _HOST[key] = ad.host_parse(ln, W)
        out.append(_HOST[key])
    return out


def device_parse(torch, lines, W, pad_front=0, pad_back=True):
    """lines back to back behind pad_front bytes, through lc_apsara_parse_device; every output is sentinel-guarded on both sides.
    pad_back False: the buffer ends on the 16-byte unit that holds the last line's last byte"""
    from loongcollector_amd import apsara
    n = len(lines)
    blob = b"#" * pad_front + b"".join(lines)
    size = (len(blob) + 15) // 16 * 16 + (16 if pad_back else 0)
    data = np.frombuffer(blob + b"]" * (size - len(blob)), np.uint8).copy()
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in lines])
    off += pad_front
    dev = torch.device("cuda:0")
    G = 4  # guard rows
    shapes = {"status": ((n + 2 * G,), torch.uint8), "secs": ((n + 2 * G,), torch.int64), "nanos": ((n + 2 * G,), torch.int32),
              "base": ((n + 2 * G, 4, 2), torch.int32), "npairs": ((n + 2 * G,), torch.int32), "pairs": ((n + 2 * G, max(W, 1), 3), torch.int32)}
    full = {k: torch.full(s, SENT % 256 if t == torch.uint8 else SENT, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    d_out = {k: v[G:G + n] for k, v in full.items()}
    apsara.parse_device(torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), n, W, d_out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in full.items()}
    for k, v in got.items():
        want = SENT % 256 if v.dtype == np.uint8 else SENT
        assert (v[:G] == want).all() and (v[G + n:] == want).all(), "%s: a guard row was written" % k
    return {k: v[G:G + n] for k, v in got.items()}


def compare(lines, W, got, what):
    rows = host_rows(lines, W)
    for i, (ln, (st, secs, ns, base, npairs, pairs)) in enumerate(zip(lines, rows)):
        where = "%s: line %d %r" % (what, i, ln[:80])
        assert int(got["status"][i]) == st, where
        assert int(got["secs"][i]) == secs and int(got["nanos"][i]) % 2 ** 32 == ns, where
        assert np.array_equal(got["base"][i].reshape(8), base), where
        assert int(got["npairs"][i]) % 2 ** 32 == npairs, where
        k = min(npairs, W)
        assert np.array_equal(got["pairs"][i][:k], pairs), where


def test_fixture_lines_device_and_host_entry(fixture_lines):
    torch = _torch()
    from loongcollector_amd import apsara
    for W in (16, 400):
        compare(fixture_lines, W, device_parse(torch, fixture_lines, W), "device W=%d" % W)
        got = apsara.parse_host(fixture_lines, W, fill=SENT)
        compare(fixture_lines, W, got, "host entry W=%d" % W)


@pytest.mark.parametrize("zone", ["UTC", "CST-8", "EST5EDT,M3.2.0,M11.1.0"])
def test_fixture_groups_equal_the_reference(fixtures, zone):
    _torch()
    from loongcollector_amd import apsara
    from loongcollector_amd.processor import EventGroup
    ref, unit = fixtures
    L = apsara._lib()

    def run(p, text):
        g = EventGroup(text.decode("latin-1"))
        rc = L.lc_apsara_processor_process(p.h, g._h)
        return rc, g.to_json()
    old = os.environ.get("TZ")
    bad, replayed = [], 0
    try:
        for r in ad.fixture_runs(ref, unit):
            if r[1] != zone:
                continue
            b, p = ad.check_run(L, ref["now"], r, process=run)
            bad += b
            replayed += p.replayed()[0]
    finally:
        if old is None:
            os.environ.pop("TZ", None)
            ad._libc.tzset()
            L.lc_timestamp_zone_reset()
        else:
            ad.set_zone(L, old)
    assert not bad, "\n".join(bad[:20])
    assert replayed > 0


def test_misaligned_outputs_are_refused():
    torch = _torch()
    from loongcollector_amd import apsara
    dev = torch.device("cuda:0")
    data = torch.zeros(64, dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 32], dtype=torch.int32, device=dev)
    raw = torch.zeros(256, dtype=torch.uint8, device=dev)
    good = {"status": raw[0:1], "secs": raw[16:24].view(torch.int64), "nanos": raw[32:36].view(torch.int32), "base": raw[64:96].view(torch.int32),
            "npairs": raw[128:132].view(torch.int32), "pairs": raw[160:172].view(torch.int32)}
    apsara.parse_device(data, off, 1, 1, good)
    torch.cuda.synchronize()
    for key, at in (("base", 68), ("secs", 20)):
        bad = dict(good)
        bad[key] = raw[at:at + good[key].numel() * good[key].element_size()]
        with pytest.raises(Exception):
            apsara.parse_device(data, off, 1, 1, bad)


def _edge_lines():
    lines = []
    # line lengths around the quad and the stage
    for n in (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129):
        body = (D + b"\t[INFO]\t[12]\t[a/b.c:7]" + b"\tk:v" * 40)[:n]
        lines.append(body)
        lines.append((b"[1378972170425093]\tkey:" + b"v" * 200)[:n])
    return lines


def test_line_counts_and_lengths():
    torch = _torch()
    base = _edge_lines()
    for n in (1, 63, 64, 65, 255, 256, 257):
        lines = [base[i % len(base)] for i in range(n)]
        compare(lines, 4, device_parse(torch, lines, 4), "n=%d" % n)


def _pad16(line):
    """the line with a last pair that brings its length to a multiple of 16: every line of a batch then starts at the batch's misalignment"""
    k = (-(len(line) + 3)) % 16
    return line + b"\tp:" + b"x" * k


def test_stage_boundaries_and_misalignment():
    torch = _torch()
    for mis in range(16):
        lines, singles = [], []
        # a base field's ']' as the last byte of a 64-byte stage (tile byte 63, 127), "\t[" opening the next
        for stage_end in (64, 128):
            fill = stage_end - mis - len(D) - len(b"\t[") - 1
            assert fill >= 0
            lines.append(_pad16(D + b"\t[" + b"A" * fill + b"]\t[12]\t[x/y:3]\tk:v\tk2:v2"))
            lines.append(_pad16(D + b"\t[" + b"A" * fill + b"]\tk:v\tk2:v2"))
            lines.append(_pad16(D + b"\t[" + b"A" * fill + b"]\n[12]\tk:v"))
            singles.append(D + b"\t[" + b"A" * fill + b"]")      # ... and the line ends there
            singles.append(D + b"\t[" + b"A" * fill + b"]\t")
        # the time's ']' and the %f digits across the boundary of stage 0: blanks move the time text to it
        for blanks in range(1, 64 - mis - 8):
            if blanks >= 64 - mis - 27:
                lines.append(_pad16(b"[2013-03-13" + b" " * blanks + b"18:05:09.493309]\t[INFO]\tk:v"))
        lines.append(_pad16(b"[1378972170" + b"4" * (60 - mis) + b"]\tk:v"))
        assert all(len(ln) % 16 == 0 for ln in lines)
        compare(lines, 4, device_parse(torch, lines, 4, pad_front=mis), "misalignment %d" % mis)
        for ln in singles:
            compare([ln], 4, device_parse(torch, [ln], 4, pad_front=mis), "misalignment %d, alone" % mis)
    # the last line ends on the buffer's last 16-byte unit, 1, 15 and 16 bytes into it
    first = _pad16(D + b"\t[INFO]\tk:v")
    for tail in (1, 15, 16):
        lines = [first, (D + b"\t[WARN]\tlast:" + b"z" * 32)[:32 + tail]]
        compare(lines, 4, device_parse(torch, lines, 4, pad_back=False), "buffer end %d" % tail)


def test_w_edges_report_the_true_count():
    torch = _torch()
    lines = [D + b"\t[INFO]" + b"".join(b"\tk%d:v%d" % (i, i) for i in range(c)) for c in (0, 1, 2, 5, 40)]
    for W in (0, 1, 4, 5, 39, 40):
        got = device_parse(torch, lines, W)  # (guard rows on both sides; a row holds exactly W triples, so a write past W lands in the next row)
        compare(lines, W, got, "W=%d" % W)
        for i, c in enumerate((0, 1, 2, 5, 40)):
            assert int(got["npairs"][i]) == c
            if W and c < W:
                assert (got["pairs"][i][c:] == SENT).all(), "a pair behind the count was written (W=%d, line %d)" % (W, i)


def test_64k_random_lines():
    torch = _torch()
    from loongcollector_amd import apsara
    rng = random.Random(20261018)
    pieces = [b"[INFO]", b"[12]", b"[a/b.c:7]", b"[]", b"[x", b"y]", b"k:v", b"key:", b":val", b"plain", b"a:b:c", b"", b"[W]", b"\n", b"content:q"]
    times = [D, b"[2013-03-13 18:05:09]", b"[1378972170425093]", b"[1378972171093]", b"[2013-3-13 8:5:9.25]", b"[bad]", b"[2013-03-13  18:05:09.25]", b"2013"]
    uniq = []
    for _ in range(2048):
        n = rng.randrange(0, 12)
        uniq.append(rng.choice(times) + b"".join(rng.choice([b"\t", b"\t", b"", b" "]) + rng.choice(pieces) for _ in range(n)))
    lines = [uniq[rng.randrange(len(uniq))] for _ in range(65536)]
    W = 6
    got = device_parse(torch, lines, W)
    compare(lines, W, got, "random")
    got = apsara.parse_host(lines[:4096], W, fill=SENT)
    compare(lines[:4096], W, got, "random, host entry")


# ---------------------------------------------------------------------------------------------- the host entry's chunk limits
def _host_equals_device(lines, W):
    """lc_apsara_parse_host against lc_apsara_parse_device over the same packed lines, on every output array; of the pairs the first
    min(npairs, W) of a line, and behind them the caller's array still holds the fill byte"""
    torch = _torch()
    from loongcollector_amd import apsara
    dev = device_parse(torch, lines, W)
    got = apsara.parse_host(lines, W, fill=SENT)
    for k in ("status", "secs", "nanos", "base", "npairs"):
        assert np.array_equal(got[k].astype(np.int64), dev[k].astype(np.int64) % 2 ** 32 if got[k].dtype == np.uint32 else dev[k]), k
    live = np.arange(W)[None, :] < np.minimum(got["npairs"], W)[:, None]
    assert np.array_equal(got["pairs"][live], dev["pairs"][live])
    assert (got["pairs"][~live].view(np.uint8) == SENT & 0xFF).all(), "a pair behind the count was written"
    compare(lines[:8] + lines[-8:], W, {k: np.concatenate([v[:8], v[-8:]]) for k, v in got.items()}, "host entry, both ends")
    return got


def test_parse_host_second_chunk_behind_two_to_the_18_lines():
    n = (1 << 18) + 1
    lines = [D + b"\t[INFO]\tk:%d" % (i % 1000) if i % 7 else b"[1378972171093]\tm:%d\tn:2\to:3" % (i % 10) for i in range(n)]
    lines[n - 1] = b"[1378972170425093]\tlast:one\tz:9"           # (the one-line second chunk; W = 4 keeps the result cap out of it)
    got = _host_equals_device(lines, 4)
    assert (int(got["status"][n - 1]), int(got["secs"][n - 1]), int(got["nanos"][n - 1]), int(got["npairs"][n - 1])) == (3, 1378972170, 425093000, 2)
    assert got["pairs"][n - 1][:2].tolist() == [[19, 23, 27], [28, 29, 31]] and (got["base"][n - 1] == -1).all()


def test_parse_host_forty_lines_of_one_mib_cross_the_payload_limit():
    head = D + b"\t[INFO]"
    lines = []
    for i in range(40):
        if i % 2:     # more pairs than W: the count is the true one, W of them come back
            m = ((1 << 20) - len(head) - 3) // 8
            body = head + b"\tkk:vvvv" * m
            body += b"\tp:" + b"x" * ((1 << 20) - len(body) - 3)
        else:
            body = head + b"\tk:" + b"v" * ((1 << 20) - len(head) - 3)
        assert len(body) == 1 << 20
        lines += [body, D + b"\t[WARN]\ts:%d" % i, b""]
    got = _host_equals_device(lines, 4)
    assert [int(c) for c in got["npairs"][:6]] == [1, 1, 0, ((1 << 20) - len(head) - 3) // 8 + 1, 1, 0]
    assert [int(s) for s in got["status"][:6]] == [5, 5, 0, 5, 5, 0]


def test_parse_host_64_mib_of_results_per_chunk_at_w_8192():
    # a line's results take W * 12 + 49 = 98353 bytes (pairs, base 32, secs 8, nanos 4, npairs 4, status 1): floor(64 MiB / 98353) = 682
    # lines fill a chunk, line 682 opens the second
    assert (64 << 20) // (8192 * 12 + 49) == 682
    lines = [D + b"\t[INFO]" + b"".join(b"\tk%d:v%d" % (c, i) for c in range(1 + i % 5)) for i in range(700)]
    got = _host_equals_device(lines, 8192)
    assert [int(c) for c in got["npairs"][678:688]] == [1 + i % 5 for i in range(678, 688)]
    assert got["pairs"][682][0].tolist() == [36, 38, 43] and got["pairs"][681][0].tolist() == [36, 38, 43]
