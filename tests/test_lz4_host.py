"""The LZ4 block writer on the CPU: the host routine of csrc/lz4_vm.hpp (the rules the kernels follow, the wavefront as a loop over 64
lanes) run by a stand-alone program (tests/native/lz4_host_check.cpp, plain and under AddressSanitizer + UBSan) over
tests/helpers/lz4_cases.py.  Every block is decoded by the strict Python decoder of tests/helpers/lz4_block.py and, where the system has
one, by liblz4's LZ4_decompress_safe; the routine is never its own reference."""
import os
import re

import pytest

from helpers import lz4_block
from helpers import lz4_cases as lc

VM = os.path.join(lc.ROOT, "loongcollector_amd", "csrc", "lz4_vm.hpp")


@pytest.fixture(scope="module")
def cases():
    return lc.cases()


@pytest.fixture(scope="module")
def blocks(cases, tmp_path_factory):
    exe = lc.build_host_check(tmp_path_factory.mktemp("lz4"))
    got, err = lc.run_host_check(exe, [(c["chunk"], c["data"]) for c in cases])
    assert err.strip() == "%d cases" % len(cases)
    return got


def test_every_block_decodes_to_its_input_within_the_bound_and_the_chunk_rule(cases, blocks):
    assert len(cases) > 100
    for c, (matches, block) in zip(cases, blocks):
        seqs = lc.check_block(block, c["data"], c["chunk"], lz4_block.decode)
        assert lz4_block.matches(seqs) == matches, c["name"]


def test_every_block_decodes_under_the_system_s_liblz4(cases, blocks):
    L = lc.system_lz4()
    if L is None:
        pytest.skip("no liblz4 on this machine: the Python decoder is the check that always runs")
    for c, (_, block) in zip(cases, blocks):
        assert lc.system_decode(L, block, len(c["data"])) == c["data"], c["name"]


def test_each_constructed_case_is_what_it_says(cases, blocks):
    seen = set()
    for c, (matches, block) in zip(cases, blocks):
        if c["expect"] is None:
            continue
        _, seqs = lz4_block.decode(block, len(c["data"]))
        kind = c["expect"][0]
        seen.add(kind)
        if kind == "nomatch":
            assert matches == [] and len(seqs) == 1, c["name"]
        elif kind == "lit":
            assert any(lit == c["expect"][1] and mlen for lit, mlen, _ in seqs), (c["name"], seqs)
        elif kind == "mlen":
            assert any(mlen == c["expect"][1] for _, mlen, _ in seqs), (c["name"], seqs)
        elif kind == "start":
            assert any(start == c["expect"][1] for start, _, _ in matches), (c["name"], matches)
        elif kind == "end":
            assert matches[-1][0] + matches[-1][1] == c["expect"][1], (c["name"], matches[-1])
    assert seen == {"nomatch", "lit", "mlen", "start", "end"}
    # the length bytes themselves: 270 literals are the token's 15 and the bytes ff 00
    block = dict((c["name"], b) for c, (_, b) in zip(cases, blocks))
    data = dict((c["name"], c["data"]) for c in cases)
    at = block["lit270"].index(data["lit270"][240:260]) - 3
    assert block["lit270"][at] >> 4 == 15 and block["lit270"][at + 1:at + 3] == b"\xff\x00"
    assert block["same0"] == b"\x00" and block["same1"] == b"\x10a"


def test_a_match_that_would_cross_a_chunk_end_stops_there(cases, blocks):
    for c, (matches, _) in zip(cases, blocks):
        if c["name"].startswith("crossing_c") and c["chunk"] > 64:
            ends = [s + n for s, n, _ in matches]
            assert c["chunk"] in ends and 2 * c["chunk"] in ends, c["name"]


def test_the_multiline_corpus_compresses_to_at_most_0_30_at_64_kib_chunks(tmp_path):
    data = lc.multiline_corpus()
    got, _ = lc.run_host_check(lc.build_host_check(tmp_path), [(65536, data), (4096, data)])
    for chunk, (_, block) in zip((65536, 4096), got):
        lc.check_block(block, data, chunk, lz4_block.decode)
    ratio = len(got[0][1]) / len(data)
    print("multiline corpus: %d bytes -> %d at 64 KiB chunks (%.3f), %d at 4 KiB" % (len(data), len(got[0][1]), ratio, len(got[1][1])))
    assert ratio <= 0.30


def test_sanitized_host_check_program(cases, blocks, tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, as a child process, once: every input an exactly-sized heap copy,
    every output exactly lz4Bound(n)"""
    got, err = lc.run_host_check(lc.build_host_check(tmp_path, sanitize=True), [(c["chunk"], c["data"]) for c in cases])
    assert got == blocks
    assert err.strip() == "%d cases" % len(cases)


def _mutant(tmp_path, old, new):
    """the check program over a scratch copy of lz4_vm.hpp with one rule changed"""
    with open(VM, encoding="utf-8") as f:
        text = f.read()
    assert text.count(old) == 1, old
    os.makedirs(tmp_path / "loongcollector_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "native")
    with open(tmp_path / "loongcollector_amd" / "csrc" / "lz4_vm.hpp", "w", encoding="utf-8") as f:
        f.write(text.replace(old, new))
    with open(os.path.join(lc.ROOT, "tests", "native", "lz4_host_check.cpp"), encoding="utf-8") as f:
        source = f.read()
    with open(tmp_path / "tests" / "native" / "lz4_host_check.cpp", "w", encoding="utf-8") as f:
        f.write(source)
    return lc.build_host_check(tmp_path, source=str(tmp_path / "tests" / "native" / "lz4_host_check.cpp"))


def _failing_cases(exe, cases):
    bad = []
    for c in cases:
        got = lc.run_host_check(exe, [(c["chunk"], c["data"])], check=False)
        if isinstance(got[0], int):
            bad.append(c["name"])
            continue
        try:
            lc.check_block(got[0][0][1], c["data"], c["chunk"], lz4_block.decode)
        except (lz4_block.Lz4BlockError, AssertionError):
            bad.append(c["name"])
    return bad


def test_mutation_dropping_the_n_minus_5_cap_fails_cases(cases, tmp_path):
    exe = _mutant(tmp_path, "return chunkEnd < n - kLz4LastLiterals ? chunkEnd : n - kLz4LastLiterals;", "return chunkEnd;")
    bad = _failing_cases(exe, [c for c in cases if re.match(r"same\d+|cut_at|period\d+$|crossing", c["name"])])
    assert "cut_at_n_minus_5" in bad and "period1" in bad and "crossing_c4096" in bad


def test_mutation_inserting_the_lanes_behind_the_hit_is_seen(cases, blocks, tmp_path):
    """the rule that only lanes <= f store: with the lanes behind f stored too, a position inside a match is in the table when the next
    step begins in front of it -- a candidate that is not in front of its position (offset 0 or worse: the program dies or the block
    does not decode) -- and the multiline corpus, where it survives, misses the ratio"""
    exe = _mutant(tmp_path, "for (uint32_t l = 0; l < 64 && l <= f; ++l) {", "for (uint32_t l = 0; l < 64; ++l) {")
    bad = _failing_cases(exe, [c for c in cases if c["name"].startswith(("text_c4096", "text_c65536", "period"))])
    assert len(bad) >= 5, bad
    corpus = {"name": "multiline", "chunk": 65536, "data": lc.multiline_corpus()}
    got = lc.run_host_check(exe, [(65536, corpus["data"])], check=False)
    assert _failing_cases(exe, [corpus]) or len(got[0][0][1]) / len(corpus["data"]) > 0.30    # the ratio case above fails under it
