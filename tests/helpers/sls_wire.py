"""The SLS LogGroup wire bytes of log events and tags, written down from sls_logs.proto and the reference's LogGroupSerializer -- a model
for the tests, with no code shared with the product.  tests/test_sls_model.py holds it to the reference's compiled writer and to a protobuf
wire decode."""


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def string_field(tag, data):
    return bytes([tag]) + varint(len(data)) + data


def pair(tag, key, value):
    """a Content (tag 0x12) or a LogTag (0x32): a message of Key = 1 and Value = 2"""
    return string_field(tag, string_field(0x0A, key) + string_field(0x12, value))


def record(time, ns, contents, enable_ns):
    """one Log: Time = 1 (never below 2^28, so that its varint has five bytes), Contents = 2, Time_ns = 4 as fixed32; b"" for no contents"""
    if not contents:
        return b""
    body = b"\x08" + varint(max(time, 1 << 28)) + b"".join(pair(0x12, k, v) for k, v in contents)
    if enable_ns and ns is not None:
        body += b"\x25" + ns.to_bytes(4, "little")
    return string_field(0x0A, body)


def records(events, enable_ns):
    """events: [(time, ns or None, [(key, value), ...])] -> the Logs fields back to back"""
    return b"".join(record(t, ns, contents, enable_ns) for t, ns, contents in events)


RESERVED_TAGS = {b"__topic__": 0x1A, b"__source__": 0x22, b"__machine_uuid__": 0x2A}


def tags(pairs):
    """Topic = 3, Source = 4, MachineUUID = 5, every other pair a LogTag = 6, in the order given"""
    return b"".join(string_field(RESERVED_TAGS[k], v) if k in RESERVED_TAGS else pair(0x32, k, v) for k, v in pairs)


def decode(data):
    """a ten-line protobuf wire decoder: [(field number, wire type, value)] with nested messages left as bytes"""
    out, at = [], 0
    while at < len(data):
        key, shift = 0, 0
        while True:
            key |= (data[at] & 0x7F) << shift
            shift += 7
            at += 1
            if data[at - 1] < 0x80:
                break
        field, wire = key >> 3, key & 7
        if wire == 0:
            value, shift = 0, 0
            while True:
                value |= (data[at] & 0x7F) << shift
                shift += 7
                at += 1
                if data[at - 1] < 0x80:
                    break
        elif wire == 2:
            n, shift = 0, 0
            while True:
                n |= (data[at] & 0x7F) << shift
                shift += 7
                at += 1
                if data[at - 1] < 0x80:
                    break
            value = data[at:at + n]
            assert len(value) == n
            at += n
        else:
            assert wire == 5, wire
            value = int.from_bytes(data[at:at + 4], "little")
            at += 4
        out.append((field, wire, value))
    return out
