"""The numpy models of tests/helpers/edge_models.py against the per-byte oracles they restate (no GPU)."""
import numpy as np

from helpers.edge_models import sched_bucket, span_filter_model, split_table_np
from helpers.pipeline_corpus import access_log_buffer
from loongcollector_amd import binding as B
from loongcollector_amd import corpus
from oracle.filter_oracle import FilterOracle
from oracle.oracle import OracleRegex
from oracle.processor_oracle import LogEventModel, ProcessorOracle
from oracle.split_oracle import split_lines, split_table

# (tests/test_gpu_pipeline.py FILTERS)
FILTERS = [
    {"FilterKey": ["user_agent"], "FilterRegex": ["^no-agent$"]},
    {"FilterKey": ["method", "response_code"], "FilterRegex": ["GET|POST", r"2\d\d"]},
    {"FilterKey": ["referrer"], "FilterRegex": [".*"]},
]


def test_split_table_np_equals_the_split_oracle():
    rng = np.random.default_rng(9)
    cases = [b"", b"x", b"\n", b"abc", b"abc\n", b"a\n\nb", b"\n\n\n", b"a" * 100, b"a\n" * 40000 + b"tail", b"ab\ncd"]
    for n in (1, 15, 16, 17, 63, 64, 65, 4097, 16384, 16385, 70000):
        cases.append(rng.choice(np.frombuffer(b"ab \n\n", dtype=np.uint8), size=n).tobytes())
    for split_char in (10, ord("a"), 0):                       # the fixed cases of tests/test_split.py
        for buf in cases:
            if split_char == 0:
                buf = buf.replace(b"b", b"\x00")
            got = split_table_np(buf, split_char)
            assert got.dtype == np.uint32 and np.array_equal(got, split_table(buf, split_char)), (split_char, len(buf))
    checked = 0
    for split_char in (10, 0, 0x80, 0xFF):
        alphabet = np.array([split_char, split_char, 0x61, 0x00, 0x0A, 0x7F, 0x80, 0xFF, 0x20], dtype=np.uint8)
        for _ in range(100):
            n = int(rng.integers(0, 5001))
            dense = rng.choice(alphabet, size=n)
            sparse = np.where(rng.random(n) < 0.002, np.uint8(split_char), np.uint8(0x62)).astype(np.uint8)
            for arr in (dense, sparse):
                buf = arr.tobytes()
                assert np.array_equal(split_table_np(buf, split_char), split_table(buf, split_char)), (split_char, n)
                assert np.array_equal(split_table_np(arr, split_char), split_table(buf, split_char))
                checked += 1
    assert checked == 800


def test_sched_bucket_is_the_clamped_length_class():
    assert list(sched_bucket(np.array([0, 31, 32, 63, 8159, 8160, 8191, 8192, 70000, 0xFFFFFFFF], dtype=np.uint32))) == [
        255, 255, 254, 254, 1, 0, 0, 0, 0, 0]
    for length in range(0, 9000, 7):
        assert int(sched_bucket(length)) == 255 - min(length >> 5, 255)


def test_span_filter_model_equals_the_parse_and_filter_oracles():
    for filt, filter_cfg in enumerate(FILTERS):
        for trailing in (True, False):
            buf, _ = access_log_buffer(700, seed=5 + filt, trailing_newline=trailing)
            spans = split_lines(buf)
            lines = [(b, buf[b:b + l]) for b, l in spans]
            caps, status = OracleRegex(corpus.REGEX_B).fullmatch_batch(
                np.frombuffer(buf, dtype=np.uint8), np.array([b for b, _ in spans], np.uint32), np.array([l for _, l in spans], np.uint32))
            rules = [(rx, corpus.KEYS_B.index(key) + 1) for key, rx in zip(filter_cfg["FilterKey"], filter_cfg["FilterRegex"])]
            counts, rows = span_filter_model(lines, status, caps, rules)
            # the chain of the oracles; the file-offset key names the line an event came from
            events = [LogEventModel([("content", line), ("__file_offset__", str(b).encode())]) for b, line in lines]
            po = ProcessorOracle({"SourceKey": "content", "Regex": corpus.REGEX_B, "Keys": corpus.KEYS_B})
            parsed = po.process_group(events, file_offset_key="__file_offset__")
            kept = FilterOracle(filter_cfg).process([dict(ev.live()) for ev in parsed])
            line_of = {b: i for i, (b, _) in enumerate(lines)}
            assert sorted(rows) == [line_of[int(c["__file_offset__"])] for c in kept]
            assert counts == [len(lines), len(kept), po.counters["out_failed"], 0]
            assert len(kept) > 20 and counts[2] > 20
            for i, row in rows.items():
                assert row[:3] == [i, lines[i][0], len(lines[i][1])] and row[3:] == list(caps[i])
                for k, key in enumerate(corpus.KEYS_B):
                    assert kept[sorted(rows).index(i)][key] == lines[i][1][row[3 + 2 * k]:row[4 + 2 * k]]


def test_span_filter_model_counts_undecided_lines_and_gives_absent_groups_the_empty_value():
    rx = OracleRegex(r"(\S+)(?: (\d+))? (.*)")
    texts = [b"a 12 rest", b"a rest of it", b"nospace", b"b 7 x", b"c  y"]
    lines, at = [], 0
    for t in texts:
        lines.append((at, t))
        at += len(t) + 1
    caps = np.full((len(texts), 6), -1, dtype=np.int32)
    status = np.zeros(len(texts), dtype=np.uint8)
    for i, t in enumerate(texts):
        m = rx.fullmatch(t)
        if m is not None:
            status[i] = B.LC_MATCH
            caps[i] = [x for be in m[1:] for x in be]
    assert list(status) == [1, 1, 0, 1, 1] and list(caps[1, 2:4]) == [-1, -1]
    assert span_filter_model(lines, status, caps, [(r"\d*", 2)])[0] == [5, 4, 1, 0]
    counts, rows = span_filter_model(lines, status, caps, [(r"\d+", 2)])
    assert counts == [5, 2, 1, 0] and sorted(rows) == [0, 3]
    status[0], status[3] = B.LC_OVERFLOW, B.LC_GAVE_UP
    assert span_filter_model(lines, status, caps, [])[0] == [5, 2, 1, 2]
