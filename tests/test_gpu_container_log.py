"""processor_parse_container_log_gpu on the device: clog_containerd_kernel and clog_docker_kernel over every fixture line through
lc_container_log_parse_device and lc_container_log_parse_host against the per-line routines compiled for the host, the processor over
every fixture group (the stdout chains among them) against the recorded output of the reference's own processor, the edges of the stage
walk at the smallest shapes that can break, sentinel-guarded outputs and shadow, and 64 Ki seeded random lines of each format."""
import ctypes
import random

import numpy as np
import pytest

from helpers import container_log_product as cp

pytestmark = pytest.mark.gpu
SENT = 0xA5
POSITIONS = (0, 15, 16, 17, 62, 63, 64, 65, 127, 128)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fixtures():
    return cp.load_fixtures()


@pytest.fixture(scope="module")
def fixture_lines(fixtures):
    lines = cp.all_lines(*fixtures) + [(cp.DOCKER, e["line"].encode("latin-1")) for e in fixtures[0]["defined_only"]]
    return {fmt: [ln for f, ln in lines if f == fmt] for fmt in (cp.CONTAINERD, cp.DOCKER)}


_HOST = {}


def host_rows(fmt, lines):
    """the per-line routine on the host (shadow pre-filled with the sentinel), once per line"""
    out = []
    for ln in lines:
        key = (fmt, ln)
        if key not in _HOST:
            _HOST[key] = cp.host_parse(fmt, ln)
        out.append(_HOST[key])
    return out


def device_parse(torch, fmt, lines, pad_front=0, pad_back=True):
    """lines back to back behind pad_front bytes, through lc_container_log_parse_device; every output array is sentinel-guarded on both
    sides and the shadow is pre-filled with the sentinel.  pad_back False: the buffer ends on the 16-byte unit that holds the last
    line's last byte.  -> the arrays, and the shadow cut into the lines' parts"""
    from loongcollector_amd import container_log
    n = len(lines)
    blob = b"#" * pad_front + b"".join(lines)
    size = max((len(blob) + 15) // 16 * 16 + (16 if pad_back else 0), 16)
    data = np.frombuffer(blob + b'"' * (size - len(blob)), np.uint8).copy()
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in lines])
    off += pad_front
    dev = torch.device("cuda:0")
    G = 4  # guard rows
    shapes = {"status": ((n + 2 * G,), torch.uint8), "flags": ((n + 2 * G,), torch.uint8), "spans": ((n + 2 * G, 3, 2), torch.int32),
              "rewrite_begin": ((n + 2 * G,), torch.int32)}
    full = {k: torch.full(s, SENT if t == torch.uint8 else -7, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    d_out = {k: v[G:G + n] for k, v in full.items()}
    d_shadow = torch.full((size + 32,), SENT, dtype=torch.uint8, device=dev)
    container_log.parse_device(fmt, torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), n, d_out, d_shadow[16:],
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in full.items()}
    for k, v in got.items():
        want = SENT if v.dtype == np.uint8 else -7
        assert (v[:G] == want).all() and (v[G + n:] == want).all(), "%s: a guard row was written" % k
    shadow = d_shadow.cpu().numpy()
    assert (shadow[:16 + pad_front] == SENT).all() and (shadow[16 + int(off[n]):] == SENT).all(), "the shadow was written outside the lines"
    res = {k: v[G:G + n] for k, v in got.items()}
    res["shadow"] = [bytes(shadow[16 + off[i]:16 + off[i + 1]]) for i in range(n)]
    return res


def compare(fmt, lines, got, what, host_entry=False):
    for i, (ln, (st, fl, spans, rb, shadow)) in enumerate(zip(lines, host_rows(fmt, lines))):
        where = "%s: line %d %r" % (what, i, ln[:100])
        assert int(got["status"][i]) == st and int(got["flags"][i]) == fl, where
        assert np.array_equal(got["spans"][i], spans) and int(got["rewrite_begin"][i]) == rb, where
        if fmt != cp.DOCKER:
            assert set(got["shadow"][i]) <= {SENT}, where
            continue
        if host_entry:  # only [rewrite_begin, content end) of a rewritten line that needs no replay comes back
            want = bytearray(b"\xa5" * len(ln))
            if st != cp.FAIL_JSON and fl & cp.ESCAPED and not fl & cp.REPLAY:
                want[rb:spans[2][1]] = shadow[rb:spans[2][1]]
            assert got["shadow"][i] == bytes(want), where
        else:  # the routine's own writes, nothing else
            assert got["shadow"][i] == shadow, where
            if st != cp.FAIL_JSON and fl & cp.ESCAPED and not fl & cp.REPLAY:
                assert set(shadow[:rb]) <= {SENT} and set(shadow[spans[2][1]:]) <= {SENT}, where


def host_entry(fmt, lines):
    from loongcollector_amd import container_log
    got = container_log.parse_host(fmt, lines, fill=SENT)
    at = np.concatenate([[0], np.cumsum([len(v) for v in lines])]).astype(np.int64)
    got["shadow"] = [bytes(got["shadow"][at[i]:at[i + 1]]) for i in range(len(lines))]
    return got


@pytest.mark.parametrize("fmt", [cp.CONTAINERD, cp.DOCKER])
def test_fixture_lines_device_and_host_entry(fixture_lines, fmt):
    torch = _torch()
    lines = fixture_lines[fmt]
    assert len(lines) > 150
    compare(fmt, lines, device_parse(torch, fmt, lines), "device")
    got = host_entry(fmt, lines)
    compare(fmt, lines, got, "host entry", host_entry=True)
    if fmt == cp.DOCKER:
        assert got["moved"] > 0
    plain = [ln for ln, row in zip(lines, host_rows(fmt, lines)) if not row[1] & cp.ESCAPED]
    assert len(plain) > 50 and host_entry(fmt, plain)["moved"] == 0


def _real_library():
    from loongcollector_amd import container_log
    from loongcollector_amd.processor import EventGroup
    L = container_log._lib()
    return L, EventGroup, container_log


def _group_json(L, g):
    """the group as fixture JSON, bytes as latin-1 (a "\\ud83d" leaves bytes that are no UTF-8)"""
    p = L.lc_group_to_json(g._h)
    try:
        return ctypes.string_at(p).decode("latin-1")
    finally:
        L.lc_free(p)


def test_fixture_groups_and_chains_equal_the_reference(fixtures):
    torch = _torch()
    from loongcollector_amd import binding
    L, EventGroup, container_log = _real_library()
    dev = torch.device("cuda:0")

    def run(p, text):
        g = EventGroup(text.decode("latin-1"))
        rc = L.lc_container_log_processor_process(p.h, g._h)
        return rc, _group_json(L, g)

    def chain(p, fmt, data):
        # the product's split on the device, the group the splitter leaves, this processor, the product's flag-mode merge
        n = len(data)
        d_data = torch.from_numpy(np.frombuffer(data + b"\0" * (64 - n % 64), np.uint8).copy()).to(dev)
        d_off = torch.zeros(n + 2, dtype=torch.int32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        d_scratch = torch.empty(binding.split_scratch_bytes(n) // 4 + 1, dtype=torch.int32, device=dev)
        binding.split_lines_device(d_data, n, d_off, d_n, d_scratch, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        nl = int(d_n.cpu()[0])
        off = d_off.cpu().numpy()[:nl + 1].astype(np.uint32)
        g = EventGroup.from_lines(np.frombuffer(data, np.uint8), off[:-1], off[1:] - off[:-1] - 1)
        container_log.set_group_format(g, fmt)
        rc = L.lc_container_log_processor_process(p.h, g._h)
        assert L.lc_merge_multiline_process_group(p.merge_handle(), L.lc_group_native(g._h)) == 0
        return rc, _group_json(L, g)

    binding.launched_kernels()
    bad, replayed, chains = [], 0, 0
    for r in cp.fixture_runs(*fixtures):
        bd, p = cp.check_run(r, L=L, process=run, chain_fn=chain)
        bad += bd
        replayed += p.replayed()
        chains += bool(r[3])
    assert not bad, "\n".join(bad[:20])
    assert replayed > 0 and chains >= 5
    launched = binding.launched_kernels()
    assert "clog_containerd_kernel" in launched and "clog_docker_kernel" in launched


def test_misaligned_outputs_and_unknown_formats_are_refused():
    torch = _torch()
    from loongcollector_amd import container_log
    dev = torch.device("cuda:0")
    data = torch.zeros(64, dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 32], dtype=torch.int32, device=dev)
    raw = torch.zeros(256, dtype=torch.uint8, device=dev)
    shadow = torch.zeros(64, dtype=torch.uint8, device=dev)
    good = {"status": raw[0:1], "flags": raw[8:9], "spans": raw[64:88].view(torch.int32), "rewrite_begin": raw[128:132].view(torch.int32)}
    for fmt in (cp.CONTAINERD, cp.DOCKER):
        container_log.parse_device(fmt, data, off, 1, good, shadow)
    torch.cuda.synchronize()
    for key, at in (("spans", 68), ("spans", 65), ("rewrite_begin", 130)):
        bad = dict(good)
        bad[key] = raw[at:at + good[key].numel() * good[key].element_size()]
        for fmt in (cp.CONTAINERD, cp.DOCKER):
            with pytest.raises(Exception):
                container_log.parse_device(fmt, data, off, 1, bad, shadow)
    for fmt in (0, 3):
        with pytest.raises(Exception):
            container_log.parse_device(fmt, data, off, 1, good, shadow)
    with pytest.raises(Exception):
        container_log.parse_device(cp.DOCKER, data, off, 1, good, None)


def _aligned(lines):
    """a filler line behind every line brings the next one to the same misalignment as the first"""
    out = []
    for ln in lines:
        out += [ln, b"x" * ((-len(ln)) % 16)]
    return out


def _containerd_edges(head):
    lines = []
    for P in POSITIONS:
        # the first blank, the second blank, the tag byte and the third blank at tile position P
        for role in (0, 7, 8, 9):
            L = P - head - role
            if L < 0:
                continue
            for src, tag in ((b"stdout", b"P "), (b"stderr", b"F "), (b"stdout", b"PP "), (b"stdout", b"X"), (b"stdoux", b"P "), (b"stdout", b" ")):
                lines.append(b"T" * L + b" " + src + b" " + tag + b"content")
        # a line that ends at tile position P: every cut of a header that lies around it
        for L in range(max(P - head - 10, 0), P - head + 2):
            for tag in (b"P ", b"F "):
                lines.append((b"T" * L + b" stdout " + tag + b"cc")[:P - head + 1])
    return lines


ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t", b"\\q", b"\\u00e9", b"\\ud83d", b"\\u0000", b"\\u 7f", b"\\u0x9z", b"\\uG123",
           b"\\u-001"]
TAIL = b'","stream":"stdout","time":"2024-02-19T03:49:37.793533014Z"}'


def _docker_edges(head):
    lines = []
    for P in (62, 63, 64, 127, 128):  # the backslash at tile position P, every escape kind
        k = P - head - 8
        for e in ESCAPES:
            lines.append(b'{"log":"' + b"a" * k + e + b"b" + TAIL)
    for P in range(58, 65):  # "\u" whose four bytes straddle the stage border
        k = P - head - 8
        lines.append(b'{"log":"' + b"a" * k + b"\\u00e9\\u12G4\\n" + TAIL)
        lines.append(b'{"stream":"stdout","time":"t","log":"' + b"a" * max(P - head - 37, 0) + b"\\u12\"}")
    for k in range(20, 30):  # a backslash as the last byte before the closing brace, across the border
        lines.append(b'{"stream":"stdout","time":"t","log":"' + b"a" * k + b"\\}")
    for k in range(44, 64):  # blank runs and key names across the border
        lines.append(b"{" + b" " * (k - head if k >= head else k) + b'"log"  :  "x\\ty"  ,  "stream" : "stderr" , "time":"t"  }')
        lines.append(b'{"time":"' + b"t" * (k - head if k >= head else k) + b'","stream":"stdout","log":"z\\n"}')
    for P in (63, 64, 65, 127, 128):  # the closing brace at tile position P
        k = P - head - len(b'{"stream":"stdout","time":"t","log":""')
        lines.append(b'{"stream":"stdout","time":"t","log":"' + b"a" * k + b'"}')
        lines.append(b'{"stream":"stdout","time":"t","log":"' + b"a" * (k - 1) + b'" }')
    # one line fails early, the others of the wave go on
    lines += [b"x" + b'{"log":"' + b"a" * 150 + TAIL, b'{"log":"\\n' + b"a" * 200 + TAIL, b'{"lo', b""]
    return lines


@pytest.mark.parametrize("fmt", [cp.CONTAINERD, cp.DOCKER])
def test_stage_walk_edges_at_every_line_head(fmt):
    torch = _torch()
    for head in range(16):
        lines = _aligned(_containerd_edges(head) if fmt == cp.CONTAINERD else _docker_edges(head))
        assert all((len(a) + len(b)) % 16 == 0 for a, b in zip(lines[::2], lines[1::2]))
        for pad_back in (True, False):
            compare(fmt, lines, device_parse(torch, fmt, lines, pad_front=head, pad_back=pad_back), "head %d, pad_back %s" % (head, pad_back))
    # (some of the shapes above must be what they are meant to be)
    rows = host_rows(cp.CONTAINERD, _containerd_edges(3))
    assert {r[0] for r in rows} == {cp.OK, cp.FAIL_TIME, cp.FAIL_SOURCE, cp.FAIL_STREAM} and any(r[1] & cp.PARTIAL for r in rows)
    rows = host_rows(cp.DOCKER, _docker_edges(3))
    assert {r[0] for r in rows} == {cp.OK, cp.FAIL_JSON} and any(r[1] & cp.ESCAPED for r in rows)


def test_containerd_long_headers_long_contents_and_tiny_lines():
    torch = _torch()
    short = b"2024-01-05T23:28:06.818486411+08:00 stdout P part"
    long_header = b"T" * 200 + b" stderr F late header"
    big = b"2024-01-05T23:28:06.818486411+08:00 stdout P " + b"c" * 16384
    for lines in ([short] * 40 + [long_header] + [short] * 23, [long_header] * 40 + [short] + [long_header] * 23,
                  [big, short, big + b" ", b"", b" ", b"x", short, big[:16000]], [b""] * 3 + [b" "] * 3, [b"x" * 20000, short]):
        compare(cp.CONTAINERD, lines, device_parse(torch, cp.CONTAINERD, lines), "%d lines" % len(lines))
        compare(cp.CONTAINERD, lines, device_parse(torch, cp.CONTAINERD, lines, pad_front=5, pad_back=False), "%d lines, head 5" % len(lines))


@pytest.mark.parametrize("fmt", [cp.CONTAINERD, cp.DOCKER])
def test_line_counts(fixture_lines, fmt):
    torch = _torch()
    from loongcollector_amd import container_log
    base = fixture_lines[fmt]
    for n in (0, 1, 63, 64, 65, 256, 257):
        lines = [base[(7 * i) % len(base)] for i in range(n)]
        compare(fmt, lines, device_parse(torch, fmt, lines), "n=%d" % n)
    assert container_log.parse_host(fmt, [])["moved"] == 0


@pytest.mark.parametrize("fmt", [cp.CONTAINERD, cp.DOCKER])
def test_64k_random_lines(fmt):
    torch = _torch()
    rng = random.Random(20261019 + fmt)
    uniq = []
    if fmt == cp.CONTAINERD:
        for _ in range(2048):
            parts = [rng.choice([b"2024-01-05T23:28:06.818486411+08:00", b"", b"t", b"x" * rng.randrange(140)]),
                     rng.choice([b"stdout", b"stderr", b"stdou", b"stdoutx", b"", b"std out"]),
                     rng.choice([b"P ", b"F ", b"P", b"F", b"PP ", b"", b" ", b"X "]) + b"c" * rng.randrange(90)]
            uniq.append(rng.choice([b" ", b" ", b" ", b"  ", b""]).join(parts))
    else:
        pieces = [b"a", b"bc", b" ", b"x" * 30, b"\\n", b"\\t", b'\\"', b"\\\\", b"\\/", b"\\b", b"\\q", b"\\u00e9", b"\\ud83d", b"\\u 7f", b"\\uG123",
                  b"\\u-001", b"\\u0000", b"{", b"}", b",", b":"]
        for _ in range(2048):
            log = b"".join(rng.choice(pieces) for _ in range(rng.randrange(0, 14)))
            keys = [(b"log", log), (b"stream", rng.choice([b"stdout", b"stderr", b"stdxx", b""])), (b"time", rng.choice([b"t", b"2024-02-19T03:49:37Z"]))]
            rng.shuffle(keys)
            if rng.random() < 0.2:
                keys.append((b"log", b"dup" + rng.choice(pieces)))
            text = b"{"
            for k, (name, val) in enumerate(keys):
                sp = rng.choice([b"", b"", b" ", b"  "])
                text += b'"' + name + b'"' + sp + b":" + sp + b'"' + val + b'"' + sp + (b"," if k < 2 else b"")
            text += b"}"
            if rng.random() < 0.06:
                text = text[:rng.randrange(len(text))]
            uniq.append(text)
    lines = [uniq[rng.randrange(len(uniq))] for _ in range(65536)]
    compare(fmt, lines, device_parse(torch, fmt, lines), "random")
    compare(fmt, lines[:4096], host_entry(fmt, lines[:4096]), "random, host entry", host_entry=True)


# ---------------------------------------------------------------------------------------------- the host entry's chunk limits
def _host_equals_device(fmt, lines):
    """lc_container_log_parse_host against lc_container_log_parse_device over the same packed lines, on every output array; of the
    shadow the host entry brings [rewrite_begin, content end) of every rewritten line that needs no replay, and nothing else"""
    torch = _torch()
    from loongcollector_amd import container_log
    dev = device_parse(torch, fmt, lines)
    got = container_log.parse_host(fmt, lines, fill=SENT)
    for k in container_log.OUT_KEYS:
        assert np.array_equal(got[k], dev[k]), k
    at = np.concatenate([[0], np.cumsum([len(v) for v in lines])]).astype(np.int64)
    want = np.full(int(at[-1]), SENT, np.uint8)
    rewritten = 0
    if fmt == cp.DOCKER:
        moves = (got["status"] != cp.FAIL_JSON) & ((got["flags"] & (cp.ESCAPED | cp.REPLAY)) == cp.ESCAPED)
        for i in np.flatnonzero(moves):
            b, e = int(got["rewrite_begin"][i]), int(got["spans"][i][2][1])
            want[at[i] + b:at[i] + e] = np.frombuffer(dev["shadow"][i][b:e], np.uint8)
            rewritten += max(e - b, 0)
    assert np.array_equal(got["shadow"], want)
    assert got["moved"] >= rewritten and (got["moved"] > 0) == (rewritten > 0)
    return got, at


def test_parse_host_containerd_second_chunk_behind_two_to_the_18_lines():
    n = (1 << 18) + 1
    lines = [b"2026-10-19T10:00:%02d.5Z %s %sline %d" % (i % 60, b"stderr" if i % 7 == 0 else b"stdout", b"P " if i % 5 == 0 else b"F ", i % 1000)
             for i in range(n)]
    lines[n - 1] = b"2026-10-19T10:00:05.000000005Z stdout F line 5"
    got, _ = _host_equals_device(cp.CONTAINERD, lines)
    assert (int(got["status"][n - 1]), int(got["flags"][n - 1]), int(got["rewrite_begin"][n - 1])) == (0, 0, 0)
    assert got["spans"][n - 1].tolist() == [[0, 30], [31, 37], [40, 46]]
    assert int(got["flags"][n - 5]) == 2 and got["moved"] == 0           # (line 2^18 - 4: partial)


def test_parse_host_docker_second_chunk_carries_an_escape_into_the_callers_shadow():
    n = (1 << 18) + 1
    lines = [b'{"log":"tab\\t%d\\n","stream":"stdout","time":"2026-10-19T10:00:05.5Z"}' % (i % 1000) if i % 5 == 0 else
             b'{"log":"plain %d","stream":"stdout","time":"2026-10-19T10:00:05.5Z"}' % (i % 1000) for i in range(n)]
    lines[n - 1] = b'{"log":"last\\tline\\n","stream":"stderr","time":"2026-10-19T10:00:05.5Z"}'     # (the one-line second chunk)
    got, at = _host_equals_device(cp.DOCKER, lines)
    assert (int(got["status"][n - 1]), int(got["flags"][n - 1]), int(got["rewrite_begin"][n - 1])) == (0, cp.ESCAPED | 1, 12)
    assert got["spans"][n - 1].tolist() == [[48, 70], [32, 38], [8, 18]]
    assert bytes(got["shadow"][at[n - 1] + 12:at[n - 1] + 18]) == b"\tline\n" and got["moved"] > 0
    assert int(got["flags"][n - 2]) == 0 and int(got["flags"][n - 5]) == cp.ESCAPED


@pytest.mark.parametrize("fmt", [cp.CONTAINERD, cp.DOCKER])
def test_parse_host_forty_lines_of_one_mib_cross_the_payload_limit(fmt):
    lines = []
    for i in range(40):
        if fmt == cp.CONTAINERD:
            head = b"2026-10-19T10:00:05.5Z stdout F "
            body = head + b"v" * ((1 << 20) - len(head))
            lines += [body, b"2026-10-19T10:00:05.5Z stderr P s%d" % i, b""]
        else:    # every other 1 MiB line escaped, at its end
            tail = b'","stream":"stdout","time":"2026-10-19T10:00:05.5Z"}'
            esc = b"\\t%d\\n" % i if i % 2 else b""
            body = b'{"log":"' + b"v" * ((1 << 20) - 8 - len(esc) - len(tail)) + esc + tail
            lines += [body, b'{"log":"s%d","stream":"stderr","time":"2026-10-19T10:00:05.5Z"}' % i, b""]
        assert len(body) == 1 << 20
    got, at = _host_equals_device(fmt, lines)
    assert [int(s) for s in got["status"][:2]] == [0, 0] and int(got["status"][2]) != 0
    if fmt == cp.DOCKER:
        assert [int(f) & cp.ESCAPED for f in got["flags"][:6]] == [0, 0, 0, cp.ESCAPED, 0, 0] and got["moved"] > 0
