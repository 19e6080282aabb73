"""Writes tests/golden/lz4_block_vectors.json (run by hand on a machine with liblz4: python tests/golden/gen_lz4_vectors.py).

"vectors": inputs with the block LZ4_compress_default of the system's liblz4 (through ctypes) makes of them -- recorded results, no
program text.  A small input is stored in hex; a large one is named by its generator of tests/helpers/lz4_cases.py, its length and its
seed, with a digest of the bytes.  "broken": hand-made blocks, one per refusal of tests/helpers/lz4_block.decode, each with the raw size
the server would be told and the reason the decoder must name.  The writer asserts that the decoder decodes every vector and refuses
every broken block for its reason."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from helpers import lz4_block  # noqa: E402
from helpers import lz4_cases as lc  # noqa: E402

GENERATED = [("text", 20000, 3), ("periodic255", 70000, 4), ("text", 4097, 5)]


def generate(gen, n, seed):
    return lc.text(n, seed) if gen == "text" else lc.periodic(int(gen[len("periodic"):]), n, seed)


def sequence(literals, offset=None, mlen=0):
    def ext(v):
        out = bytearray()
        if v >= 15:
            v -= 15
            while v >= 255:
                out.append(255)
                v -= 255
            out.append(v)
        return bytes(out)
    lit = len(literals)
    if offset is None:
        return bytes([min(lit, 15) << 4]) + ext(lit) + literals
    return bytes([min(lit, 15) << 4 | min(mlen - 4, 15)]) + ext(lit) + literals + bytes([offset & 255, offset >> 8]) + ext(mlen - 4)


def broken_blocks(valid, valid_n):
    return [
        {"name": "offset_0", "n": 16, "block": sequence(b"abcd", 0, 7) + sequence(b"efghi"), "reason": "offset 0"},
        {"name": "offset_beyond_output", "n": 16, "block": sequence(b"abcd", 5, 7) + sequence(b"efghi"), "reason": "offset beyond"},
        {"name": "no_closing_sequence", "n": 24, "block": sequence(b"abcdefghijkl", 4, 12), "reason": "no closing literal-only sequence"},
        {"name": "last_match_too_late", "n": 17, "block": sequence(b"abcdefgh", 4, 4) + sequence(b"ijklm"), "reason": "last match starts after n - 12"},
        {"name": "four_closing_literals", "n": 20, "block": sequence(b"abcd", 4, 12) + sequence(b"wxyz"), "reason": "fewer than 5 closing literals"},
        {"name": "truncated", "n": valid_n, "block": valid[:-2], "reason": "truncated"},
        {"name": "trailing_bytes", "n": valid_n, "block": valid + b"\x00", "reason": "trailing bytes"},
    ]


def main():
    L = lc.system_lz4()
    assert L is not None, "this writer needs the system's liblz4"
    vectors = []
    small = [c for c in lc.cases() if len(c["data"]) <= 700 and c["chunk"] == 65536]
    for c in small:
        vectors.append({"name": c["name"], "input": c["data"].hex(), "block": lc.system_compress(L, c["data"]).hex()})
    for gen, n, seed in GENERATED:
        data = generate(gen, n, seed)
        vectors.append({"name": "%s_%d_%d" % (gen, n, seed), "gen": gen, "n": n, "seed": seed, "input_sha256": hashlib.sha256(data).hexdigest(),
                        "block": lc.system_compress(L, data).hex()})
    sample = lc.text(300, 1)
    broken = [dict(b, block=b["block"].hex()) for b in broken_blocks(lc.system_compress(L, sample), len(sample))]
    for v in vectors:
        data = bytes.fromhex(v["input"]) if "input" in v else generate(v["gen"], v["n"], v["seed"])
        assert lz4_block.decode(bytes.fromhex(v["block"]), len(data))[0] == data, v["name"]
    for b in broken:
        try:
            lz4_block.decode(bytes.fromhex(b["block"]), b["n"])
        except lz4_block.Lz4BlockError as e:
            assert b["reason"] in str(e), (b["name"], str(e))
        else:
            raise AssertionError("decoded: " + b["name"])
    path = os.path.join(HERE, "lz4_block_vectors.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"liblz4": "LZ4_compress_default of the build machine's liblz4.so.1", "vectors": vectors, "broken": broken}, f, separators=(",", ":"))
    print("%d vectors, %d broken blocks, %d bytes" % (len(vectors), len(broken), os.path.getsize(path)))


if __name__ == "__main__":
    main()
