"""A small Python restatement of the delimiter parser: the trim, the four-state quote machine, the plain split with its two quirks, and
the processor's column rules.  It is an oracle for large random batches on a GPU box (where the reference does not exist) ONLY because
tests/test_delimiter_model.py first holds it to every case of tests/golden/delimiter_reference_outputs.json, the reference's own output.

Lines and values are bytes.  split_line mirrors the device's output: (status, true column count, [(begin, end, doubled)])."""

FAIL, OK, BLANK = 0, 1, 2


class Engine:
    def __init__(self, separator, quote=b'"', mode="extend", n_keys=0):
        self.sep = bytes(separator)
        self.quote = bytes(quote)[:1]
        self.mode = mode
        self.n_keys = n_keys
        self.use_quote = len(self.sep) == 1 and self.quote != self.sep

    def trim(self, line):
        end = len(line)
        while end > 0 and line[end - 1] in b" \r":
            end -= 1
        begin = 0
        while begin < end and line[begin] == 0x20:
            begin += 1
        return begin, end

    def split_line(self, line):
        begin, end = self.trim(line)
        if len(line) == 0 or begin >= end:
            return BLANK, 0, []
        return self._quoted(line, begin, end) if self.use_quote else self._plain(line, begin, end)

    def _plain(self, line, begin, end):
        cols = []
        d = len(self.sep)
        pos = begin
        while True:
            at = line.find(self.sep, pos, end)
            if at < 0:
                cols.append((pos, end, False))
                break
            cols.append((pos, at, False))
            pos = at + d
            if self.mode != "extend" and len(cols) >= self.n_keys:
                cols.append((at, end, False))      # the remainder starts AT the separator
                break
        return OK, len(cols), cols

    def _quoted(self, line, begin, end):
        sep, quote = self.sep[0], self.quote[0]
        cols = []
        i = begin
        while True:
            # one field starts at i
            if i < end and line[i] == quote:
                start = i + 1
                j = start
                doubled = False
                while True:
                    j = line.find(self.quote, j, end)
                    if j < 0:
                        return FAIL, 0, []          # the line ends inside the quotes
                    if j + 1 < end and line[j + 1] == quote:
                        doubled = True
                        j += 2
                        continue
                    break
                cols.append((start, j, doubled))
                j += 1                               # behind the closing quote: a separator or the end
                if j >= end:
                    break
                if line[j] != sep:
                    return FAIL, 0, []
                i = j + 1
            else:
                j = line.find(self.sep, i, end)
                if j < 0:
                    j = end
                if line.find(self.quote, i, j) >= 0:
                    return FAIL, 0, []              # a quote inside an unquoted field
                cols.append((i, j, False))
                if j >= end:
                    break
                i = j + 1
        return OK, len(cols), cols

    def value(self, line, col):
        b, e, doubled = col
        v = line[b:e]
        return v.replace(self.quote + self.quote, self.quote) if doubled else v


class Processor:
    """config: the plugin's JSON object (str values); process(lines) -> (events' contents, counters, alarms)"""

    def __init__(self, config):
        c = config
        sep = c["Separator"]
        if sep == "\\t":
            sep = "\t"
        self.source = c["SourceKey"].encode()
        self.keys = [k.encode() for k in c["Keys"]]
        self.mode = c.get("OverflowedFieldsTreatment") or "extend"
        if self.mode not in ("extend", "keep", "discard"):
            self.mode = "extend"
        quote = c.get("Quote") or '"'
        self.engine = Engine(sep.encode("latin-1"), quote.encode("latin-1") if len(sep) == 1 else b'"', self.mode, len(self.keys))
        if len(sep) > 1:
            self.engine.use_quote = False
        self.allow_short = bool(c.get("AllowingShortenedFields", False))
        self.keep_fail = bool(c.get("KeepingSourceWhenParseFail", False))
        self.keep_ok = bool(c.get("KeepingSourceWhenParseSucceed", False))
        self.renamed = (c.get("RenamedSourceKey") or c["SourceKey"]).encode()
        self.copy_raw = bool(c.get("CopingRawLog", False))
        self.overwritten = self.source in self.keys
        self.counters = [0, 0, 0, 0]   # discarded, out_failed, out_key_not_found, out_successful
        self.alarms = []

    @staticmethod
    def _set(contents, key, value, overwrite=True):
        for kv in contents:
            if kv[0] == key:
                if overwrite:
                    kv[1] = value
                return
        contents.append([key, value])

    def process_event(self, contents):
        """contents: [[key, value], ...] (bytes), changed in place; False: the event is dropped"""
        raw = None
        for k, v in contents:
            if k == self.source:
                raw = v
        if raw is None:
            self.counters[2] += 1
            return True
        status, n, cols = self.engine.split_line(raw)
        if status == BLANK:
            self.counters[1] += 1
            return True
        K = len(self.keys)
        ok = status == OK
        values = [self.engine.value(raw, c) for c in cols]
        if ok:
            if self.engine.use_quote and self.mode != "extend" and n > K:
                values = values[:K] + [b"".join(self.engine.sep + v for v in values[K:])]
                n = K + 1
            if n == 0 or (not self.allow_short and n < K):
                self.alarms.append(b"keys count unmatch columns count :%d, required:%d, logs:" % (n, K) + raw)
                ok = False
        else:
            self.alarms.append(b"parse delimiter log fail, logs:" + raw)
        if ok:
            for idx in range(n):
                if idx < K:
                    if self.mode == "discard" and self.keys[idx] == b"_":
                        continue
                    self._set(contents, self.keys[idx], values[idx])
                elif self.mode != "discard":
                    self._set(contents, b"__column%d__" % idx, values[idx])
            self.counters[3] += 1
        else:
            self.counters[1] += 1
        if not ok or not self.overwritten:
            contents[:] = [kv for kv in contents if kv[0] != self.source]
        if (ok and self.keep_ok) or (not ok and self.keep_fail):
            self._set(contents, self.renamed, raw, overwrite=False)
        if not ok and self.keep_fail and self.copy_raw:
            self._set(contents, b"__raw_log__", raw, overwrite=False)
        if not ok and not self.keep_fail and not contents:
            self.counters[0] += 1
            return False
        return True

    def process(self, events):
        return [ev for ev in events if self.process_event(ev)]
