"""The deterministic corpus of the field codecs, used on the CPU (tests/test_codec_model.py, tests/test_codec_host.py) and on the GPU
(tests/test_gpu_codec.py): [(residue of the value's first byte, value)] per op, and the build / run of the stand-alone host program."""
import json
import os
import subprocess

from helpers import codec_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VECTORS = os.path.join(ROOT, "tests", "golden", "codec_unittest_vectors.json")
BORDERS = (15, 16, 17, 63, 64, 65, 255, 256, 257)  # tile offsets: unit, stage and 256-byte borders
LENGTHS = sorted(set(range(41)) | {e + d for e in (48, 64, 128, 192, 256, 512) for d in range(-2, 3)})
MD5_LENGTHS = sorted(set(LENGTHS) | {55, 56, 57, 63, 64, 65, 119, 120, 121})
SKIPS = (b"\r", b"\n", b"\r\n")


def load_vectors():
    with open(VECTORS, encoding="utf-8") as f:
        return json.load(f)


def payload(n, salt=0):
    """n bytes that run through all 256 byte values"""
    return bytes((i * 37 + salt * 101 + 13) & 255 for i in range(n))


def text64(n, salt=0):
    """n alphabet bytes"""
    return bytes(model.ALPHABET[(i * 29 + salt * 7 + 3) % 64] for i in range(n))


def encode_cases(lengths=LENGTHS):
    return [(r, payload(n, r & 3)) for n in lengths for r in range(16)]  # (four payloads per length: the model's answers are cached)


def md5_cases():
    return encode_cases(MD5_LENGTHS)


def mime(data, line=76, sep=b"\r\n"):
    text = model.encode(data)
    return b"".join(text[i:i + line] + sep for i in range(0, len(text), line))


def _on_borders(make, shortest=0):
    """make(index) -> a value whose deciding byte stands at `index` of the value; for every tile offset of BORDERS and every residue"""
    out = []
    for t in BORDERS:
        for r in range(16):
            if t - r >= shortest:
                out.append((r, make(t - r)))
    return out


def decode_clean_cases():
    return [(r, model.encode(v)) for r, v in encode_cases()]


def decode_skip_cases():
    out = []
    base = model.encode(payload(229, 3))          # 308 characters, ends in "=="
    base1 = model.encode(payload(230, 4))         # ends in "="
    base0 = model.encode(payload(231, 5))         # no padding
    assert base.endswith(b"==") and base1.endswith(b"=") and not base1.endswith(b"==") and not base0.endswith(b"=")
    for skip in SKIPS:
        for text in (base, base1, base0):
            out += _on_borders(lambda i, text=text, skip=skip: text[:i] + skip + text[i:])
        for r in range(16):
            for text in (base, base1, base0, model.encode(payload(r + 1, r))):
                out.append((r, skip + text))                        # at the start
                out.append((r, text + skip))                        # at the end, behind the padding
                out.append((r, text + skip + skip))
            out.append((r, base[:-1] + skip + b"="))                # between the two `=`
            out.append((r, base[:-1] + skip + b"=" + skip))
            out.append((r, base[:-2] + skip + b"=" + skip + skip + b"=" + skip))
            out.append((r, skip))                                   # nothing but CR/LF: the empty value
    for r in range(16):
        for n in (1, 56, 57, 58, 114, 115, 229, 570, 3000):         # MIME: 76 characters + CRLF
            out.append((r, mime(payload(n, r))))
            out.append((r, mime(payload(n, r), sep=b"\n")))
        out.append((r, mime(payload(100, r), line=1)))              # a CRLF behind every character
    return out


def decode_error_cases():
    out = []
    body = text64(400, 1)

    def quanta(i):
        """i alphabet bytes"""
        return body[:i]

    # a non-alphabet byte: the deciding byte on the borders
    for bad in (b"-", b"_", b"\x00", b"\x80", b"\xff", b" ", b"\t"):
        out += _on_borders(lambda i, bad=bad: quanta(i) + bad + body[i:300])
    # values that END on the borders: 1, 2 and 3 trailing characters without padding (and whole quanta, which decode)
    out += _on_borders(lambda i: quanta(i + 1))
    # `=` at every j, the deciding `=` on the borders: j = 0 / 1 are errors, j = 2 alone at the end, j = 2 followed by x, j = 3
    out += _on_borders(lambda i: quanta(i) + b"=")
    out += _on_borders(lambda i: quanta(i) + b"==")
    out += _on_borders(lambda i: quanta(i) + b"=x")
    out += _on_borders(lambda i: quanta(i) + b"=x=")
    out += _on_borders(lambda i: quanta(i) + b"=\r\nx")       # (Go's quirk: q - 1 is the LF's position)
    out += _on_borders(lambda i: quanta(i) + b"=\r\n")
    # trailing garbage behind `=` and `==`: the garbage on the borders
    def garbage_at(i, pad, garbage):
        """(line feeds in front so that) whole quanta, 2 or 3 characters and `pad` end right in front of index i"""
        want = 3 if pad == b"=" else 2
        m = i - len(pad)
        whole = m - (m - want) % 4
        return b"\n" * (m - whole) + quanta(whole) + pad + garbage

    for pad in (b"=", b"=="):
        for garbage in (b"A", b"=", b"\x00"):
            out += _on_borders(lambda i, pad=pad, garbage=garbage: garbage_at(i, pad, garbage), shortest=8)
    for tail in (b"A", b"=", b"-", b"\r\nA", b"A\r\n"):
        for r in range(16):
            for n in (2, 3, 14, 15, 62, 63, 254, 255):
                out.append((r, quanta(n) + (b"==" if n % 4 == 2 else b"=") + tail))
    # two errors in one value: the first wins
    out += _on_borders(lambda i: quanta(i) + b"-" + body[i:i + 40] + b"_" + body[:9])
    out += _on_borders(lambda i: quanta(i) + b"\x80" + b"====")
    for r in range(16):
        out.append((r, b"="))
        out.append((r, b"=="))
        out.append((r, b"A"))
        out.append((r, b"A==="))
        out.append((r, b"\r\n=\r\n"))
        out.append((r, b"QQ=\r\n"))
    return out


def decode_special_cases():
    out = []
    for r in range(16):
        # non-canonical trailing bits: not checked
        out += [(r, b"QR=="), (r, b"QQ=="), (r, b"QUJ="), (r, b"QUH="), (r, text64(60, r) + b"Q/=="), (r, text64(252, r) + b"QU/=")]
        out.append((r, b""))
    for c in range(256):                                             # every byte value: as a payload byte, and as a character
        out.append((c % 16, model.encode(bytes([c]) * (1 + c % 5))))
        out.append((c % 16, b"QUJD" + bytes([c]) + b"REVG"))
        out.append((c % 16, text64(15 - c % 16 + 16) + bytes([c])))
    out.append((3, model.encode(bytes(range(256)))))
    return out


def decode_cases():
    return decode_clean_cases() + decode_skip_cases() + decode_error_cases() + decode_special_cases()


def cases(op):
    return {"base64_encode": encode_cases, "md5": md5_cases, "base64_decode": decode_cases}[op]()


# ---------------------------------------------------------------------------------------------- the stand-alone host program
OP_CODE = {"base64_encode": 0, "base64_decode": 1, "md5": 2}


def build_host_check(out_dir, sanitize=False):
    exe = os.path.join(str(out_dir), "codec_host_check_asan" if sanitize else "codec_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + ["-o", exe, os.path.join(ROOT, "tests", "native", "codec_host_check.cpp")])
    return exe


def run_host_check(exe, path, pairs):
    """pairs: [(op, value)], written to the file `path` -> the program's lines"""
    with open(path, "wb") as f:
        for op, value in pairs:
            f.write(b"%d %d\n" % (OP_CODE[op], len(value)) + value + b"\n")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode("utf-8", "replace")[-2000:])
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(pairs)
    return out


def expected_text(op, value):
    """the line the host program prints for a value the routines get right"""
    flags, out, err = model.apply(op, value)
    if flags & model.ERROR:
        return "2 @%d" % err
    return "1 %s" % (out.hex() if out else "=")
