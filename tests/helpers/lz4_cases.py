"""TEST INFRASTRUCTURE ONLY: the inputs the LZ4 block writer is held to (tests/test_lz4_host.py on the host routine, tests/test_gpu_lz4.py
on the device), each with what it was constructed to show, and the helpers that build and run tests/native/lz4_host_check.cpp."""
import ctypes
import ctypes.util
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

END_LENGTHS = [0, 1, 4, 5, 11, 12, 13, 14, 16, 17, 63, 64, 65]
LITERAL_RUNS = [14, 15, 16, 269, 270, 271, 524, 525]
MATCH_LENGTHS = [4, 18, 19, 20, 273, 274, 275]
PERIODS = [1, 2, 3, 5, 63, 64, 65, 70, 255, 256]
CHUNKS = [64, 4096, 65536]


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def text(n, seed):
    """compressible bytes: words of a small vocabulary"""
    rng = random.Random(seed)
    words = [b"GET", b"POST", b"/api/v1/orders", b"/index.html", b"200", b"404", b"timeout", b"upstream", b"10.0.0.", b"request", b"served in"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" " + (b"%d " % rng.randrange(1000) if rng.random() < 0.3 else b"")
    return bytes(out[:n])


def periodic(period, n, seed):
    unit = rnd(period, seed)
    return (unit * (n // period + 1))[:n]


def _slot(data, p):
    """lz4Hash of csrc/lz4_vm.hpp on the four bytes at p"""
    return (int.from_bytes(data[p:p + 4], "little") * 2654435761 & 0xFFFFFFFF) >> 20


def _source_survives(data, source, copy):
    """no position between a copy's source and the copy takes the source's table entry"""
    return all(_slot(data, q) != _slot(data, source) for q in range(source + 1, copy))


def literal_run_case(run, seed):
    """a match of 40 that a chosen byte ends at 240, `run` literals (that byte the first), then a match: a literal run of exactly `run`"""
    while True:
        base = rnd(200, seed)
        lits = bytes([base[40] ^ 0xFF]) + rnd(run - 1, seed + 1)
        data = base + base[:40] + lits + base[100:140] + bytes([base[140] ^ 0xFF]) + rnd(20, seed + 2)
        if _source_survives(data, 0, 200) and _source_survives(data, 100, 240 + run):
            return data
        seed += 1000


def match_length_case(mlen, seed):
    """a copy of `mlen` bytes of the head, ended by a chosen byte"""
    while True:
        base = rnd(400, seed)
        data = base + rnd(70, seed + 1) + base[50:50 + mlen] + bytes([base[50 + mlen] ^ 0xFF]) + rnd(20, seed + 2)
        if _source_survives(data, 50, 470):
            return data
        seed += 1000


def cases():
    """[{name, chunk, data, expect}]: expect is None, ("lit", L): a sequence with L literals and a match, ("mlen", M): a match of M,
    ("start", S): a match that starts at S, ("nomatch",): a block of literals only, ("end", E): the last match ends at E"""
    out = []

    def add(name, chunk, data, expect=None):
        out.append({"name": name, "chunk": chunk, "data": data, "expect": expect})
    for n in END_LENGTHS:
        add("same%d" % n, 65536, b"a" * n, ("nomatch",) if n < 13 else None)
        add("random%d" % n, 65536, rnd(n, 100 + n), ("nomatch",))
    add("cut_at_n_minus_5", 65536, b"ab" * 100, ("end", 195))
    for run in LITERAL_RUNS:
        add("lit%d" % run, 65536, literal_run_case(run, 200 + run), ("lit", run))
    for mlen in MATCH_LENGTHS:
        add("mlen%d" % mlen, 65536, match_length_case(mlen, 300 + mlen), ("mlen", mlen))
    for period in PERIODS:
        add("period%d" % period, 65536, periodic(period, 1000, 400 + period))
        add("period%d_c4096" % period, 4096, periodic(period, 9000, 400 + period))
        add("period%d_c64" % period, 64, periodic(period, 1000, 400 + period))
    for c in CHUNKS:
        for n in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 7):
            add("text_c%d_n%d" % (c, n), c, text(n, n))
        # a run of one period that would cross every chunk end: each chunk's match stops there
        # (a chunk of 64 bytes is one step on an empty table: it never finds a match)
        add("crossing_c%d" % c, c, periodic(7, 3 * c, 5), ("end", 3 * c - 5) if c > 64 else ("nomatch",))
        add("random_between_c%d" % c, c, text(c, 1) + rnd(c, 2) + text(c, 3))
        add("random_first_c%d" % c, c, rnd(c, 4) + text(2 * c, 5))
        add("random_last_c%d" % c, c, text(2 * c, 6) + rnd(c, 7))
        add("all_random_c%d" % c, c, rnd(3 * c, 8), ("nomatch",))
        head = rnd(64, 9)
        add("hit_lane0_c%d" % c, c, head + head[:8] + rnd(40, 10), ("start", 64) if c > 64 else ("nomatch",))
        add("hit_lane63_c%d" % c, c, head + rnd(63, 11) + head[:8] + rnd(40, 12), ("start", 127) if c > 64 else ("nomatch",))
        add("short_step_c%d" % c, c, text(c + 20, 13))  # the last step of each chunk has fewer than 64 lanes
    return out


def multiline_corpus():
    from loongcollector_amd import corpus
    return corpus.multiline_buffer(150000)


# ---- the stand-alone program
def build_host_check(out_dir, sanitize=False, source=None):
    exe = os.path.join(str(out_dir), "lz4_host_check_asan" if sanitize else "lz4_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + ["-o", exe, source or os.path.join(ROOT, "tests", "native", "lz4_host_check.cpp")])
    return exe


def run_host_check(exe, items, check=True):
    """items: [(chunk, data)] -> [(matches [(start, len, offset)], block bytes)], stderr; check=False: -> the return code instead when
    the program fails"""
    payload = b"".join(b"C %d %d\n" % (chunk, len(data)) + data + b"\n" for chunk, data in items)
    r = subprocess.run([exe], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if r.returncode != 0 and not check:
        return r.returncode, r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, (r.returncode, r.stderr.decode("utf-8", "replace")[-2000:])
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == 2 * len(items)
    out = []
    for m, hexed in zip(lines[0::2], lines[1::2]):
        flat = [int(x) for x in m.split(" ")[1:]]
        out.append((list(zip(flat[0::3], flat[1::3], flat[2::3])), bytes.fromhex(hexed)))
    return out, r.stderr.decode()


# ---- the system's liblz4, where there is one
def system_lz4():
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    L = ctypes.CDLL(name)
    L.LZ4_decompress_safe.restype = ctypes.c_int
    L.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    L.LZ4_compress_default.restype = ctypes.c_int
    L.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    L.LZ4_compressBound.restype = ctypes.c_int
    L.LZ4_compressBound.argtypes = [ctypes.c_int]
    return L


def system_decode(L, block, n):
    buf = ctypes.create_string_buffer(max(1, n))
    got = L.LZ4_decompress_safe(block, buf, len(block), n)
    return buf.raw[:got] if got >= 0 else None


def system_compress(L, data):
    cap = L.LZ4_compressBound(len(data))
    buf = ctypes.create_string_buffer(max(1, cap))
    got = L.LZ4_compress_default(data, buf, len(data), cap)
    assert got > 0
    return buf.raw[:got]


def check_block(block, data, chunk, decode):
    """what every block must obey beyond decoding to its input: the bound, the chunk rule"""
    got, seqs = decode(block, len(data))
    assert got == data
    assert len(block) <= len(data) + len(data) // 255 + 16
    at = 0
    for lit, mlen, offset in seqs:
        at += lit
        if mlen:
            assert offset < chunk and (at - offset) // chunk == at // chunk == (at + mlen - 1) // chunk, (at, mlen, offset)
        at += mlen
    return seqs
