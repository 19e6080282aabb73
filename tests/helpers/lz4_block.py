"""TEST INFRASTRUCTURE ONLY: a strict decoder of one LZ4 block (block format, no frame) in plain Python -- the check that always runs,
beside the system's liblz4 where there is one.  It knows the raw size n, as the server does from the request header."""


class Lz4BlockError(ValueError):
    pass


def decode(block, n):
    """-> (the n bytes, [(literal_len, match_len, offset), ...]); the closing sequence has match_len 0 and offset 0.  Refuses, with the
    reason in the message: "offset 0", "offset beyond the bytes produced", "no closing literal-only sequence", "last match starts after
    n - 12", "fewer than 5 closing literals", "truncated", "trailing bytes", "size"."""
    out = bytearray()
    seqs = []
    at = 0
    size = len(block)

    def length(nibble):
        nonlocal at
        v = nibble
        if nibble == 15:
            while True:
                if at >= size:
                    raise Lz4BlockError("truncated: length bytes")
                b = block[at]
                at += 1
                v += b
                if b != 255:
                    break
        return v

    while True:
        if at >= size:
            raise Lz4BlockError("truncated: no token" if not seqs else "no closing literal-only sequence")
        token = block[at]
        at += 1
        lit = length(token >> 4)
        if at + lit > size:
            raise Lz4BlockError("truncated: literals")
        out += block[at:at + lit]
        at += lit
        if len(out) > n or (len(out) == n and at < size):
            raise Lz4BlockError("trailing bytes")
        if at == size:  # the closing sequence: literals only
            if token & 15:
                raise Lz4BlockError("no closing literal-only sequence")
            if seqs and lit < 5:
                raise Lz4BlockError("fewer than 5 closing literals")
            seqs.append((lit, 0, 0))
            break
        if at + 2 > size:
            raise Lz4BlockError("truncated: offset")
        offset = block[at] | block[at + 1] << 8
        at += 2
        mlen = length(token & 15) + 4
        if offset == 0:
            raise Lz4BlockError("offset 0")
        if offset > len(out):
            raise Lz4BlockError("offset beyond the bytes produced")
        start = len(out)
        if start + 12 > n:
            raise Lz4BlockError("last match starts after n - 12")
        if start + mlen > n:
            raise Lz4BlockError("size: a match runs beyond n")
        if offset >= mlen:
            out += out[start - offset:start - offset + mlen]
        else:
            for i in range(mlen):
                out.append(out[start - offset + i])
        seqs.append((lit, mlen, offset))
    if len(out) > n:
        raise Lz4BlockError("trailing bytes")
    if len(out) < n:
        raise Lz4BlockError("truncated: %d of %d bytes" % (len(out), n))
    return bytes(out), seqs


def matches(seqs):
    """[(start, match_len, offset)] of a sequence list"""
    out, at = [], 0
    for lit, mlen, offset in seqs:
        at += lit
        if mlen:
            out.append((at, mlen, offset))
        at += mlen
    return out
