"""The cases of the strrep tests, each a (config, value) pair: the reference's unit-test strings (tests/golden/strrep_unittest_vectors.json),
named shapes at the borders the kernels walk over (16-byte units, 64-byte stages, tile positions counted from the 16-byte boundary at or
below a value's first byte), and seeded corpora; and the stand-alone host program that walks csrc/strrep_vm.hpp over them.  The expected
answer is always tests/helpers/strrep_model.py's, computed live."""
import json
import os
import random
import subprocess

from helpers import strrep_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VECTORS = os.path.join(ROOT, "tests", "golden", "strrep_unittest_vectors.json")
UNQUOTE = {"SourceKey": "content", "Method": "unquote"}
BORDERS = (15, 16, 17, 63, 64, 65, 127, 128, 129)
NEEDLES = ("#", "ab", "abc", "0123456789abcdef", "0123456789abcdefg", "0123456789abcdefghijklmnopqrstuv")
ESCAPES = (b"\\a", b"\\\\", b'\\"', b"\\x41", b"\\xff", b"\\101", b"\\u554a", b"\\U0001F600")
UTF8 = ("é".encode(), "啊".encode(), "\U0001F600".encode())


def const(match, repl=""):
    return {"SourceKey": "content", "Method": "const", "Match": match, "ReplaceString": repl}


def load_vectors():
    with open(VECTORS, encoding="utf-8") as f:
        return json.load(f)


def filler(n, salt=0):
    """n bytes that hold no needle of NEEDLES, no quote, no backslash, no newline"""
    return bytes(b"zyxwvZYXWV.,;:"[(i * 7 + salt) % 14] for i in range(n))


def at_tile_offsets(piece, which, total=150, wrap=False):
    """values of `total` filler bytes with `piece` placed so that its byte `which` (an index into piece) stands on every tile offset of
    BORDERS, for all 16 residues of the value's first byte -> [(residue, value)].  wrap: the value is put into quotes (form A)."""
    out = []
    for t in BORDERS:
        for r in range(16):
            index = t - r - which - (1 if wrap else 0)
            if index < 0:
                continue
            body = filler(index, t) + piece + filler(max(0, total - index - len(piece)), r)
            out.append((r, b'"' + body + b'"' if wrap else body))
    return out


def const_border_cases():
    """the first and the last byte of an occurrence on every border, every residue, needles of 1, 2, 3, 16, 17 and 32 bytes"""
    out = []
    for k, needle in enumerate(NEEDLES):
        config = const(needle, ("", "R", needle[::-1], "<" + "r" * 62 + ">")[k % 4])
        n = needle.encode()
        for which in sorted({0, len(n) - 1}):
            out += [(config, r, v) for r, v in at_tile_offsets(n, which)]
    return out


def const_shape_cases():
    out = []
    for needle in NEEDLES[1:]:
        n = needle.encode()
        for repl in ("", "R", "=" * len(n), "r" * 64):
            config = const(needle, repl)
            for t in (16, 64):
                for r in (0, 5, 15):
                    i = t - r - (len(n) - 1)  # the needle's last byte on the border ...
                    if i < 0:
                        continue
                    out.append((config, r, filler(i) + n[:-1] + b"!" + filler(40)))  # ... but it is a near miss, one byte short
                    out.append((config, r, filler(i) + n[:-1]))                       # cut by the value's end
                    out.append((config, r, filler(i) + n))                            # ends with the value
                    out.append((config, r, filler(i) + n + n + filler(9)))            # back to back across the border
                    out.append((config, r, filler(i) + n[:1] + n + filler(9)))
            out.append((config, 0, n * 7))                                            # only occurrences
            out.append((config, 3, n))
    for needle, runs in (("aa", b"a"), ("aba", b"ab")):
        for repl in ("", "X", "aaaa", "aba"):
            config = const(needle, repl)
            for t in (16, 64, 128):
                for r in (0, 1, 7, 15):
                    for back in range(0, 6):  # a run that starts `back` bytes in front of the border: the cover crosses it
                        i = t - r - back
                        if i < 0:
                            continue
                        for count in (2, 3, 4, 5, 9):
                            out.append((config, r, filler(i) + (runs * 40)[:count + (count if len(runs) > 1 else 0)] + filler(20)))
    out.append((const("aa", "b"), 0, b"aaaaa"))
    out.append((const("#", "r" * 256), 0, b"#" * 48))
    out.append((const("#"), 9, b"#" * 100))
    return out


def unquote_border_cases():
    out = []
    for esc in ESCAPES + (b'"',):
        for which in sorted({0, len(esc) // 2, len(esc) - 1}):
            out += [(UNQUOTE, r, v) for r, v in at_tile_offsets(esc, which, total=140)]
            if esc != b'"':
                out += [(UNQUOTE, r, v) for r, v in at_tile_offsets(esc, which, total=140, wrap=True)]
    # a backslash run of 1 to 5 in front of `"`, x41, u0041, n and the value's end; the run's first, middle and last backslash on every
    # border, every residue, forms A and B (behind the value's end: the run ends the value, or the content of form A)
    for run in range(1, 6):
        for behind in (b'"', b"x41", b"u0041", b"n", b""):
            piece = b"\\" * run + behind
            for which in sorted({0, run // 2, run - 1}):
                for wrap in (False, True):
                    for r, v in at_tile_offsets(piece, which, total=0 if behind == b"" else 100, wrap=wrap):
                        out.append((UNQUOTE, r, v))
    out.append((UNQUOTE, 0, b'a\\"b'))  # the quirk: a literal backslash in front of x22
    return out


def unquote_error_cases():
    """every error rule once, and errors whose deciding byte is the first byte of the next unit"""
    singles = [b'"', b'"a"b"', b"a\\", b'"a\\"', b"a\nb", b"\\'", b"\\x4", b"\\x4g", b"\\400", b"\\12", b"\\128", b"\\ud800", b"\\udfff",
               b"\\U00110000", b"\\U0010FFF", b"\\u55", b"\\q", b"\\x", b"\\", b'"\n"', b'"\\x4"', b"\\Uffffffff", b"\\0", b'"ab\\q"']
    out = [(UNQUOTE, 0, s) for s in singles]
    for lead, decider in ((b"\\x4", b"g"), (b"\\", b"q"), (b"\\u00e", b"-"), (b"\\U0010FFF", b"x"), (b"\\12", b"8"), (b"\\", b"'"), (b"", b"\n"),
                          (b"\\4", b"00")):
        for t in (16, 64, 128):
            for r in (0, 3, 15):
                index = t - r - len(lead)
                if index >= 0:
                    out.append((UNQUOTE, r, filler(index) + lead + decider + filler(5)))
                    out.append((UNQUOTE, r, b'"' + filler(index - 1) + lead + decider + b'"') if index >= 1 else (UNQUOTE, r, lead + decider))
    return out


def unquote_utf8_cases():
    out = []
    for seq in UTF8:
        for which in range(len(seq)):
            out += [(UNQUOTE, r, v) for r, v in at_tile_offsets(seq, which, total=140)]
        for cut in range(1, len(seq)):  # cut by the value's end, every byte of the cut piece on every border, every residue
            for t in BORDERS:
                for r in range(16):
                    for which in range(cut):
                        index = t - r - which
                        if index >= 0:
                            out.append((UNQUOTE, r, filler(index) + seq[:cut]))
                            out.append((UNQUOTE, r, b'"' + filler(index) + seq[:cut] + b'"'))
                            out.append((UNQUOTE, r, filler(index) + seq[:cut] + b"z" + seq))
    for bad in (b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\x80", b"\xff", b"\xc1\xbf", b"\xf5\x80\x80\x80"):
        for r in (0, 14, 15):
            out.append((UNQUOTE, r, bad))
            out.append((UNQUOTE, r, filler(16 - r) + bad + filler(3)))
            out.append((UNQUOTE, r, filler(15 - r if r < 15 else 0) + bad + bad))
    out.append((UNQUOTE, 5, b"\xff" * 64))  # 192 bytes
    out.append((UNQUOTE, 0, b"\xe4\xb8"))   # six bytes
    return out


def unquote_special_cases():
    out = [(UNQUOTE, 0, b'""'), (UNQUOTE, 0, b'"'), (UNQUOTE, 0, b""), (UNQUOTE, 15, b'""'), (UNQUOTE, 15, b'"'), (UNQUOTE, 15, b'"x"')]
    out += [(UNQUOTE, b % 16, bytes([b])) for b in range(256)]
    out += [(UNQUOTE, (b + 7) % 16, b"\\" + bytes([b])) for b in range(256)]
    out += [(UNQUOTE, 0, b'"\\' + bytes([b]) + b'"') for b in range(256)]
    return out


def length_cases():
    """value lengths 0 to 65 for both methods: every byte changes"""
    out = []
    for n in range(66):
        out.append((const("#", "ab"), n % 16, b"#" * n))
        out.append((const("ab", ""), (n * 5) % 16, (b"ab" * 33)[:n]))
        out.append((UNQUOTE, (n * 3) % 16, (b"\\\\" * 33)[:n]))
        out.append((UNQUOTE, n % 16, (b'\\t"' * 22)[:n]))
    return out


CONST_ALPHABETS = [
    (const("a", "bb"), [b"a", b"b", b"c"]),
    (const("aa", "a"), [b"a", b"a", b"b"]),
    (const("aba", "<>"), [b"a", b"b", b"ab"]),
    (const("abcabc", ""), [b"abc", b"ab", b"c", b"x"]),
    (const("\u001b[0;39m", ""), [b"\x1b[0;39m", b"\x1b[", b"0;39m", b"INFO ", b"\x1b"]),
    (const("0123456789abcdef0123456789abcdef", "r" * 100), [b"0123456789abcdef", b"0123456789abcde", b"f", b"-"]),
    (const("（需", "）"), ["（".encode(), "需".encode(), b"\xef\xbc", b"\x88", b"q"]),
]
UNQUOTE_ALPHABET = [b"\\", b"\\", b'"', b"x", b"u", b"U", b"n", b"t", b"0", b"1", b"2", b"7", b"4", b"f", b"F", b"d", b"8", b"a", b"z", b" ", b"'",
                    b"\n", b"\\x22", b"\\u554a", b"\\U0001f600", b"\\101", "啊".encode(), "é".encode(), "\U0001F600".encode(), b"\xe5",
                    b"\x95", b"\xff", b"\xc0", b"\xed\xa0\x80"]


def random_cases(seed, n, longest=200):
    """n seeded values per const alphabet and 4 n for the unquote, a third of those in quotes"""
    rnd = random.Random(seed)
    out = []
    for config, symbols in CONST_ALPHABETS:
        for _ in range(n):
            out.append((config, rnd.randrange(16), b"".join(rnd.choice(symbols) for _ in range(rnd.randrange(0, longest // 2)))[:longest]))
    plain = [s for s in UNQUOTE_ALPHABET if s not in (b"'", b"\n", b"\xff", b"\xc0", b"\xed\xa0\x80", b"8")]
    for k in range(4 * n):
        symbols = UNQUOTE_ALPHABET if k % 2 else plain  # (the full alphabet mostly ends in an error: half the values avoid its sure ones)
        body = b"".join(rnd.choice(symbols) for _ in range(rnd.randrange(0, longest // 3)))[:longest]
        out.append((UNQUOTE, rnd.randrange(16), b'"' + body + b'"' if k % 3 == 0 else body))
    return out


def named_cases():
    return (const_border_cases() + const_shape_cases() + unquote_border_cases() + unquote_error_cases() + unquote_utf8_cases() +
            unquote_special_cases() + length_cases())


def expected_text(config, value):
    """the host program's line for what the model says"""
    flags, out = model.apply(config, value)
    if not flags & model.CHANGED:
        return "%d -" % flags
    return "%d %s" % (flags, out.hex() if out else "=")


# ---------------------------------------------------------------------------------------------- the stand-alone host program
def build_host_check(out_dir, sanitize=False):
    exe = os.path.join(str(out_dir), "strrep_host_check_asan" if sanitize else "strrep_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + ["-o", exe, os.path.join(ROOT, "tests", "native", "strrep_host_check.cpp")])
    return exe


def run_host_check(exe, pairs):
    """pairs: [(config, value)] -> the program's lines"""
    payload = []
    for config, value in pairs:
        match = config.get("Match", "").encode("utf-8")
        repl = config.get("ReplaceString", "").encode("utf-8")
        payload.append(b"%d %d %d %d\n" % (0 if config["Method"] == "const" else 1, len(match), len(repl), len(value)) + match + repl + value + b"\n")
    r = subprocess.run([exe], input=b"".join(payload), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode("utf-8", "replace")[-2000:])
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(pairs)
    return out
