"""The strict LZ4 block decoder of the tests (tests/helpers/lz4_block.py) against liblz4's own blocks: tests/golden/lz4_block_vectors.json
holds small inputs with the block LZ4_compress_default made of them on the build machine, and hand-broken blocks, one per refusal
(tests/golden/gen_lz4_vectors.py writes the file).  The decoder is what the host routine and the device are then held to."""
import hashlib
import json
import os

import pytest

from helpers import lz4_block
from helpers import lz4_cases as lc

with open(os.path.join(lc.ROOT, "tests", "golden", "lz4_block_vectors.json"), encoding="utf-8") as f:
    GOLDEN = json.load(f)


def _input(v):
    if "input" in v:
        return bytes.fromhex(v["input"])
    data = lc.text(v["n"], v["seed"]) if v["gen"] == "text" else lc.periodic(int(v["gen"][len("periodic"):]), v["n"], v["seed"])
    assert hashlib.sha256(data).hexdigest() == v["input_sha256"], v["name"]
    return data


def test_the_decoder_decodes_every_block_of_liblz4():
    assert len(GOLDEN["vectors"]) >= 40
    with_matches = 0
    for v in GOLDEN["vectors"]:
        data = _input(v)
        got, seqs = lz4_block.decode(bytes.fromhex(v["block"]), len(data))
        assert got == data, v["name"]
        assert sum(lit + mlen for lit, mlen, _ in seqs) == len(data) and seqs[-1][1] == 0
        with_matches += len(seqs) > 1
    assert with_matches >= 15


@pytest.mark.parametrize("broken", GOLDEN["broken"], ids=[b["name"] for b in GOLDEN["broken"]])
def test_the_decoder_refuses_a_broken_block_and_names_the_reason(broken):
    with pytest.raises(lz4_block.Lz4BlockError, match=broken["reason"]):
        lz4_block.decode(bytes.fromhex(broken["block"]), broken["n"])


def test_the_broken_blocks_cover_every_refusal():
    assert {b["reason"] for b in GOLDEN["broken"]} == {"offset 0", "offset beyond", "no closing literal-only sequence", "last match starts after n - 12",
                                                        "fewer than 5 closing literals", "truncated", "trailing bytes"}
