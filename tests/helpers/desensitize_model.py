"""The reference for processor_desensitize_gpu's tests: the two loops of ProcessorDesensitizeNative::CastOneSensitiveWord as
include/lc_desensitize.h states them, over oracle.OracleRegex.search(s, start) with ORX_NO_MOD_S | ORX_NO_MOD_M | ORX_REGEXP2, the
per-event rules of ProcessEvent, and hashlib's MD5 in upper case.  `const` searches the whole value from `start`; `md5` searches
value[s:] from 0.  RE2 itself cannot be built here: what this model rests on is said in tests/golden/README_desensitize.md."""
import hashlib

from oracle.oracle import ORX_NO_MOD_M, ORX_NO_MOD_S, ORX_REGEXP2, OracleRegex

FLAGS = ORX_NO_MOD_S | ORX_NO_MOD_M | ORX_REGEXP2
CHANGED, GAVE_UP = 1, 2


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def parse_rewrite(rewrite, groups):
    """RE2::Rewrite's reading (2018-09-01) -> list of bytes (literal) and int (RE2 group) pieces; None: the error path (a backslash
    in front of anything but 0-9 and a backslash, or at the end).  A number above `groups` gives "" and is dropped."""
    pieces = []
    i = 0
    while i < len(rewrite):
        c = rewrite[i:i + 1]
        i += 1
        if c != b"\\":
            pieces.append(c)
            continue
        if i >= len(rewrite):
            return None
        d = rewrite[i:i + 1]
        i += 1
        if d == b"\\":
            pieces.append(b"\\")
        elif d.isdigit():
            if int(d) <= groups:
                pieces.append(int(d))
        else:
            return None
    return pieces


class Rule:
    def __init__(self, method, before, content, replacing=b"", replacing_all=False):
        assert method in ("const", "md5")
        self.method, self.replacing_all = method, bool(replacing_all)
        self.rx = OracleRegex(b"(" + _b(before) + b")" + _b(content), FLAGS)
        self.rewrite = parse_rewrite(b"\\1" + _b(replacing), self.rx.groups) if method == "const" else []
        self.pass_through = self.rewrite is None

    @classmethod
    def from_config(cls, config):
        return cls(config["Method"], config["ContentPatternBeforeReplacedString"], config["ReplacedContentPattern"],
                   config.get("ReplacingString", ""), config.get("ReplacingAll", False) is True)

    def cuts(self, value):
        """-> (list of (cut begin, match end, replacement bytes, groups), searches); [] for an unchanged value.  groups: the match's
        (begin, end) per RE2 group 0.., in the whole value.  Raises RuntimeError("complexity exceeded") where the oracle gives up."""
        n = len(value)
        if self.pass_through:
            return [], 0
        out, searches = [], 0
        if self.method == "const":
            p, lastend = 0, None
            while p <= n:
                m = self.rx.search(value, p)
                searches += 1
                if m is None:
                    break
                mb, me = m[0]
                if mb == me and mb == lastend:
                    p += 1
                    continue
                text = b"".join(q if isinstance(q, bytes) else (value[m[q][0]:m[q][1]] if m[q][0] >= 0 else b"") for q in self.rewrite)
                out.append((mb, me, text, m))
                p = lastend = me
                if not self.replacing_all:
                    break
            return out, searches
        s = 0
        while True:
            m = self.rx.search(value[s:], 0)
            searches += 1
            if m is None:
                break
            m = [(b + s, e + s) if b >= 0 else (b, e) for b, e in m]
            me, g = m[0][1], m[1][1]
            if me == s:
                return [], searches
            out.append((g, me, hashlib.md5(value[g:me]).hexdigest().upper().encode(), m))
            s = me
            if me >= n or not self.replacing_all:
                break
        return out, searches

    def apply(self, value):
        """-> the new value, or None for an unchanged one"""
        cuts, _ = self.cuts(value)
        if not cuts:
            return None
        return compose(value, cuts)

    def rounds(self, values):
        """match launches a batch takes on the device: the longest search sequence of a value (one with ReplacingAll off)"""
        if self.pass_through or not values:
            return 0
        return max(self.cuts(v)[1] for v in values)


def compose(value, cuts):
    out, at = [], 0
    for cut_b, me, text, _ in cuts:
        out += [value[at:cut_b], text]
        at = me
    out.append(value[at:])
    return b"".join(out)


def process_group(config, group, encoding="latin-1"):
    """ProcessEvent over a fixture group ({"events": [{"type": 1, "contents": {..}}, ..]}) -> (the group afterwards, counters):
    no log event or no SourceKey: out_failed; an empty value: out_key_not_found; every other event: out_successful"""
    rule = Rule.from_config(config)
    key = config["SourceKey"]
    counters = {"out_failed_events_total": 0, "out_key_not_found_events_total": 0, "out_successful_events_total": 0, "discarded_events_total": 0}
    events = []
    for ev in group["events"]:
        ev = dict(ev)
        if ev.get("type") != 1 or key not in ev.get("contents", {}):
            counters["out_failed_events_total"] += 1
            events.append(ev)
            continue
        contents = dict(ev["contents"])
        if contents[key] == "":
            counters["out_key_not_found_events_total"] += 1
        else:
            counters["out_successful_events_total"] += 1
            new = rule.apply(contents[key].encode(encoding))
            if new is not None:
                contents[key] = new.decode(encoding)
        ev["contents"] = contents
        events.append(ev)
    out = dict(group)
    out["events"] = events
    return out, counters
