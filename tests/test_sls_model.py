"""tests/helpers/sls_wire.py, the Python model of the SLS wire writer the GPU tests compare with, held to the REFERENCE's own writer
(core/protobuf/sls/LogGroupSerializer.cpp compiled into oracle/_ref/libref_processor.so, driven as SLSEventGroupSerializer drives it)
and to a protobuf wire decode.  Over every parser configuration of helpers/sls_cases.py: the reference's processor_parse_regex_native
runs on a generated group, its serializer writes what is left, and the model writes the same events.  While it runs here it records
tests/golden/sls_wire_vectors.json (README_sls.md): the GPU box has no reference tree, its tests use that file and the model.
CPU only; the comparisons with the reference are skipped where its tree is not present."""
import json
import os
import random

import pytest

from helpers import sls_cases as sc
from helpers import sls_wire

needs_reference = pytest.mark.skipif(not os.path.isdir(sc.REF), reason="needs the reference tree (/root/reference): its serializer is compiled from there")


def _decoded_events(data):
    """the wire bytes back as the model's events, by the wire decoder alone"""
    out = []
    for field, wire, body in sls_wire.decode(data):
        assert (field, wire) == (1, 2)
        parts = sls_wire.decode(body)
        assert parts[0][:2] == (1, 0) and parts[0][2] >= 1 << 28
        contents, ns = [], None
        for f, w, v in parts[1:]:
            if (f, w) == (2, 2):
                assert ns is None     # Time_ns stands behind the contents
                (kf, kw, key), (vf, vw, value) = sls_wire.decode(v)
                assert (kf, kw, vf, vw) == (1, 2, 2, 2)
                contents.append((key, value))
            else:
                assert (f, w) == (4, 5)
                ns = v
        out.append((parts[0][2], ns, contents))
    return out


@needs_reference
def test_the_model_equals_the_reference_on_every_configuration_and_the_golden_file_is_what_it_wrote():
    from test_reference_neighbours import RefPlugin
    vectors, total = [], 0
    for config, group, enable_ns in sc.vector_inputs():
        want = sc.reference_bytes(RefPlugin("processor_parse_regex_native", config), group, enable_ns)
        left = RefPlugin("processor_parse_regex_native", config).process(group)
        events = sc.model_events(left)
        assert sls_wire.records(events, enable_ns) == want, (config, group)
        expect = [(max(t, 1 << 28), ns if enable_ns else None, c) for t, ns, c in events if c]
        assert _decoded_events(want) == expect
        vectors.append({"config": config, "group": group, "enable_ns": enable_ns, "bytes": want.hex()})
        total += len(want)
    assert len(vectors) == 53 and total > 20000
    text = json.dumps(vectors, ensure_ascii=True, separators=(",", ":")) + "\n"
    assert len(text) < 400 << 10
    if not os.path.exists(sc.GOLDEN) or open(sc.GOLDEN, encoding="utf-8").read() != text:
        with open(sc.GOLDEN, "w", encoding="utf-8") as f:
            f.write(text)
    assert sc.load_golden() == vectors


@needs_reference
def test_the_model_equals_the_reference_s_serializer_on_random_events():
    """the serializer alone (no processor): events of 0 to 6 contents, keys and values of 0 to 20 000 bytes on both sides of 2^7 and 2^14,
    times below, at and above 2^28, with and without a nanosecond part, both flags"""
    rng = random.Random(11)
    sizes = [0, 1, 2, 100, 126, 127, 128, 129, 1000, 16381, 16382, 16383, 16384, 16385, 20000]
    for k in range(60):
        events = []
        for _ in range(rng.randint(0, 8)):
            contents = [["k%d_" % j + "x" * rng.choice(sizes[:9]), "v" * rng.choice(sizes)] for j in range(rng.randint(0, 6))]
            ev = {"contents": contents, "timestamp": rng.choice(sc.TIMES), "type": 1}
            if rng.random() < 0.6:
                ev["timestampNanosecond"] = rng.choice([0, 999999999, rng.randrange(10 ** 9)])
            events.append(ev)
        for enable_ns in (0, 1):
            want = sc.reference_bytes(None, {"events": [dict(e, contents=dict(e["contents"])) for e in events]}, enable_ns)
            assert sls_wire.records(sc.model_events(events), enable_ns) == want, (k, enable_ns)


def test_the_model_s_bytes_decode_to_what_went_in():
    """no reference needed: the model against the wire decoder, records and tags"""
    events = [(5, None, [(b"k", b"v")]), (1 << 28, 0, [(b"a" * 130, b"b" * 20000), (b"", b"")]), (1700000000, 999999999, []), ((1 << 32) - 1, 7, [(b"x", b"")])]
    for enable_ns in (0, 1):
        got = _decoded_events(sls_wire.records(events, enable_ns))
        assert got == [(max(t, 1 << 28), ns if enable_ns else None, c) for t, ns, c in events if c]
    pairs = [(b"__topic__", b"t"), (b"host", b"h" * 200), (b"__source__", b"10.0.0.1"), (b"__machine_uuid__", b"u-1"), (b"", b""), (b"__topic__", b"")]
    fields = sls_wire.decode(sls_wire.tags(pairs))
    assert [(f, w) for f, w, _ in fields] == [(3, 2), (6, 2), (4, 2), (5, 2), (6, 2), (3, 2)]
    assert fields[0][2] == b"t" and fields[2][2] == b"10.0.0.1" and fields[3][2] == b"u-1" and fields[5][2] == b""
    assert [v for _, _, v in sls_wire.decode(fields[1][2])] == [b"host", b"h" * 200] and [v for _, _, v in sls_wire.decode(fields[4][2])] == [b"", b""]


def test_the_golden_file_is_small_and_whole():
    vectors = sc.load_golden()
    assert len(vectors) == 53 and os.path.getsize(sc.GOLDEN) < 400 << 10
    assert [(v["config"], v["group"], v["enable_ns"]) for v in vectors] == [(c, g, e) for c, g, e in sc.vector_inputs()]
    assert sum(1 for v in vectors if any(len(e["contents"]) > 1 for e in v["group"]["events"])) == 1
