"""A Python model of processor_parse_timestamp_native: strptime_ns (core/common/Strptime.cpp) interpreted straight from the format
string -- NOT through the product's compiled program --, Strptime() with its three year modes (core/common/TimeUtil.cpp) on glibc's
mktime, and ParseLogTime / ProcessEvent with the per-group string cache, walked line by line.  The end of the value acts as the NUL.
tests/test_timestamp_model.py holds the model to every floor vector."""
import ctypes

INT_MIN = -2 ** 31
SPACE = b" \t\n\v\f\r"
DAY = ["Sunday", "Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday"]
MON = ["January", "February", "March", "April", "May", "June", "July", "August", "September", "October", "November", "December"]
COMPOSITE = {"c": "%a %b %d %H:%M:%S %Y", "D": "%m/%d/%y", "F": "%Y-%m-%d", "R": "%H:%M", "r": "%I:%M:%S %p", "T": "%H:%M:%S",
             "X": "%H:%M:%S", "x": "%m/%d/%y"}


class Tm(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("sec", "min", "hour", "mday", "mon", "year", "wday", "yday", "isdst")] + [
        ("gmtoff", ctypes.c_long), ("zone", ctypes.c_char_p)]


_libc = ctypes.CDLL(None)
_libc.mktime.restype = ctypes.c_int64
_libc.mktime.argtypes = [ctypes.POINTER(Tm)]
_libc.localtime_r.restype = ctypes.c_void_p
_libc.localtime_r.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Tm)]


def mktime(tm):
    return _libc.mktime(ctypes.byref(Tm(tm["sec"], tm["min"], tm["hour"], tm["mday"], tm["mon"], tm["year"], 0, 0, tm["isdst"], 0, None)))


def localtime(t):
    out = Tm()
    _libc.localtime_r(ctypes.byref(ctypes.c_int64(t)), ctypes.byref(out))
    return out


def _cdiv(a, b):  # C's division truncates toward zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _cmod(a, b):
    return a - _cdiv(a, b) * b


class _Fail(Exception):
    pass


class _State:
    def __init__(self, buf):
        self.buf, self.bp = buf, 0
        self.tm = {"sec": 0, "min": 0, "hour": 0, "mday": 0, "mon": 0, "year": INT_MIN, "isdst": 0}
        self.ns, self.ns_len = 0, -1

    def ch(self, k=0):
        i = self.bp + k
        return self.buf[i] if i < len(self.buf) else 0

    def conv_num(self, llim, ulim):
        c = self.ch()
        if not 48 <= c <= 57:
            return None
        result, rulim = 0, ulim
        while True:
            result = result * 10 + c - 48
            rulim //= 10
            self.bp += 1
            c = self.ch()
            if not (result * 10 <= ulim and rulim and 48 <= c <= 57):
                break
        return result if llim <= result <= ulim else None

    def conv_nanos(self):
        c = self.ch()
        if not 48 <= c <= 57:
            return False
        result, digits, start = 0, 0, self.bp
        while 48 <= c <= 57:
            result = (result * 10 + c - 48) & 0xffffffff
            digits += 1
            self.bp += 1
            c = self.ch()
        for _ in range(9 - digits):
            result = (result * 10) & 0xffffffff
        self.ns, self.ns_len = result, self.bp - start
        return True

    def find_string(self, *tables):
        for names in tables:
            for i, name in enumerate(names):
                n = len(name)
                if self.buf[self.bp:self.bp + n].upper() == name.upper().encode() and self.bp + n <= len(self.buf):
                    self.bp += n
                    return i
        return None

    def skip_space(self):
        while self.bp < len(self.buf) and self.buf[self.bp] in SPACE:
            self.bp += 1


def _run(s, fmt):
    """one call of strptime_ns (the '%s' special case aside); raises _Fail where the reference returns NULL"""
    tm = s.tm
    split_year = False
    s.ns = 0
    i = 0
    while i < len(fmt):
        c = fmt[i]
        i += 1
        alt = 0
        if c in " \t\n\v\f\r":
            s.skip_space()
            continue
        if c != "%":
            ok = s.ch() == ord(c)
            s.bp += 1
            if not ok:
                raise _Fail
            continue

        def legal(allowed):
            if alt & ~allowed:
                raise _Fail
        while True:
            c = fmt[i] if i < len(fmt) else "\0"
            i += 1
            if c in "EO":
                legal(0)
                alt |= 1 if c == "E" else 2
                continue
            break
        if c == "%":
            ok = s.ch() == 37
            s.bp += 1
            if not ok:
                raise _Fail
            legal(0)
        elif c in COMPOSITE:
            if c in "DFRrT":
                legal(0)
            _run(s, COMPOSITE[c])
            legal(1)
        elif c in "Aa":
            r = s.find_string(DAY, [d[:3] for d in DAY])
            if r is None:
                raise _Fail
            legal(0)
        elif c in "Bbh":
            r = s.find_string(MON, [m[:3] for m in MON])
            if r is None:
                raise _Fail
            tm["mon"] = r
            legal(0)
        elif c == "C":
            r = s.conv_num(0, 99)
            v = 20 if r is None else r
            v = v * 100 - 1900
            if split_year:
                v += _cmod(tm["year"], 100)
            split_year = True
            tm["year"] = v
            if r is None:
                raise _Fail
            legal(1)
        elif c in "de":
            r = s.conv_num(1, 31)
            if r is None:
                raise _Fail
            tm["mday"] = r
            legal(2)
        elif c == "f":
            if not s.conv_nanos():
                raise _Fail
            legal(2)
        elif c in "kH":
            if c == "k":
                legal(0)
            r = s.conv_num(0, 23)
            if r is None:
                raise _Fail
            tm["hour"] = r
            legal(2)
        elif c in "lI":
            if c == "l":
                legal(0)
            r = s.conv_num(1, 12)
            if r is not None:
                tm["hour"] = r
            if tm["hour"] == 12:
                tm["hour"] = 0
            if r is None:
                raise _Fail
            legal(2)
        elif c == "j":
            if s.conv_num(1, 366) is None:
                raise _Fail
            legal(0)
        elif c == "M":
            r = s.conv_num(0, 59)
            if r is None:
                raise _Fail
            tm["min"] = r
            legal(2)
        elif c == "m":
            r = s.conv_num(1, 12)
            tm["mon"] = (1 if r is None else r) - 1
            if r is None:
                raise _Fail
            legal(2)
        elif c == "p":
            r = s.find_string(["AM", "PM"])
            if tm["hour"] > 11:
                raise _Fail
            tm["hour"] += (r or 0) * 12
            if r is None:
                raise _Fail
            legal(0)
        elif c == "S":
            r = s.conv_num(0, 61)
            if r is None:
                raise _Fail
            tm["sec"] = r
            legal(2)
        elif c in "UW":
            if s.conv_num(0, 53) is None:
                raise _Fail
            legal(2)
        elif c == "w":
            if s.conv_num(0, 6) is None:
                raise _Fail
            legal(2)
        elif c == "u":
            if s.conv_num(1, 7) is None:
                raise _Fail
            legal(2)
        elif c == "g":
            if s.conv_num(0, 99) is None:
                raise _Fail
        elif c == "G":
            if s.bp >= len(s.buf):
                raise _Fail  # (the reference steps over the NUL: undefined there, a failure in the product)
            s.bp += 1
            while 48 <= s.ch() <= 57:
                s.bp += 1
        elif c == "V":
            if s.conv_num(0, 53) is None:
                raise _Fail
        elif c == "Y":
            r = s.conv_num(0, 9999)
            tm["year"] = (1900 if r is None else r) - 1900
            if r is None:
                raise _Fail
            legal(1)
        elif c == "y":
            r = s.conv_num(0, 99)
            v = 0 if r is None else r
            if split_year:
                v += _cdiv(tm["year"], 100) * 100
            else:
                split_year = True
                v = v + 100 if v <= 68 else v
            tm["year"] = v
            if r is None:
                raise _Fail
        elif c == "Z":
            if s.buf[s.bp:s.bp + 3].upper() in (b"GMT", b"UTC"):
                tm["isdst"] = 0
                s.bp += 3
        elif c == "z":
            s.skip_space()
            z = s.ch()
            s.bp += 1
            if z in b"GUZ":
                if z == 71:
                    ok = s.ch() == 77
                    s.bp += 1
                    if not ok:
                        raise _Fail
                if z != 90:
                    ok = s.ch() == 84
                    s.bp += 1
                    if not ok:
                        raise _Fail
                tm["isdst"] = 0
            elif z in b"+-":
                offs = n = 0
                while n < 4:
                    d = s.ch()
                    if 48 <= d <= 57:
                        offs = offs * 10 + d - 48
                        s.bp += 1
                        n += 1
                    elif n == 2 and d == 58:
                        s.bp += 1
                    else:
                        break
                if n == 4:
                    if offs % 100 >= 60:
                        raise _Fail
                elif n != 2:
                    raise _Fail
                tm["isdst"] = 0
            else:
                s.bp -= 1
                if s.find_string(["EST", "CST", "MST", "PST"]) is not None:
                    pass
                elif s.find_string(["EDT", "CDT", "MDT", "PDT"]) is not None:
                    tm["isdst"] = 1
                elif 65 <= z <= 73 or 76 <= z <= 89:
                    s.bp += 1
                else:
                    raise _Fail
        elif c in "nt":
            s.skip_space()
            legal(0)
        else:
            raise _Fail


def strptime_ns(value, fmt):
    """-> (matched or -1, tm dict, nanos, nanos_len, epoch second or None)"""
    s = _State(value)
    if fmt == "%s":
        p = 0
        while p < len(value) and value[p] in SPACE:
            p += 1
        q = p + 1 if p < len(value) and value[p] in b"+-" else p
        e = q
        while e < len(value) and 48 <= value[e] <= 57:
            e += 1
        n = int(value[p:e]) if e > q else 0
        n = max(min(n, 2 ** 63 - 1), -2 ** 63)
        text = str(n)
        keep = min(len(text), 10)
        for _ in range(len(text) - keep):
            n = _cdiv(n, 10)
        if n == 0:
            return -1, s.tm, 0, -1, None
        s.ns, s.ns_len = 0, 0
        s.bp = keep
        s.conv_nanos()
        return e, s.tm, s.ns, s.ns_len, n
    try:
        _run(s, fmt)
    except _Fail:
        return -1, s.tm, s.ns, s.ns_len, None
    return s.bp, s.tm, s.ns, s.ns_len, None


def Strptime(value, fmt, now, year_mode=-1):
    """TimeUtil.cpp:141-190 -> (matched or -1, tv_sec or None (left alone), nanos, nanos_len)"""
    matched, tm, ns, ns_len, epoch = strptime_ns(value, fmt)
    if fmt == "%f":
        return matched, None, ns, ns_len
    if epoch is not None:
        return matched, epoch, ns, ns_len  # mktime(localtime(t)) = t
    if year_mode >= 0 and tm["year"] == INT_MIN:
        if year_mode > 0:
            tm["year"] = year_mode - 1900
        else:
            cur = localtime(now)
            if tm["mon"] == 0 and tm["mday"] == 1 and cur.mon == 11 and cur.mday == 31:
                tm["year"] = cur.year + 1
            elif tm["mon"] == 11 and tm["mday"] == 31 and cur.mon == 0 and cur.mday == 1:
                tm["year"] = cur.year - 1
            else:
                tm["year"] = cur.year
    return matched, mktime(tm), ns, ns_len


def zone_offset(source_timezone, now):
    """ParseLogTimeZoneOffsetSecond -> offset, or None when the string is not valid"""
    tz = source_timezone
    if not tz:
        return 0
    if len(tz) != 9 or tz[6] != ":" or tz[3] not in "+-" or not tz.startswith("GMT"):
        return None

    def two(t):
        if t.isdigit():
            return int(t)
        if t[0] == "-" and t[1].isdigit():
            return -int(t[1])
        return None
    h, m = two(tz[4:6]), two(tz[7:9])
    if h is None or m is None:
        return None
    sec = h * 3600 + m * 60
    return (-sec if tz[3] == "-" else sec) - localtime(now).gmtoff


class Processor:
    """Process / ProcessEvent / ParseLogTime, one event at a time"""

    def __init__(self, config, now, discard=True, interval=43200):
        self.fmt, self.now = config["SourceFormat"], now
        self.year = config.get("SourceYear", -1)
        self.offset = zone_offset(config.get("SourceTimezone", ""), now) or 0
        self.discard, self.interval = discard, interval
        self.counters = {"discarded": 0, "out_failed": 0, "key_not_found": 0, "out_successful": 0, "history_failure": 0}
        self.alarms = []

    def process_values(self, values):
        at = self.fmt.find("%f")
        have, at_end = at >= 0, at >= 0 and at == len(self.fmt) - 2
        cache, tv_sec, out = b"", 0, []
        for text in values:
            v = text.encode("latin-1")
            ns = 0
            if (not have or at_end) and cache and v.startswith(cache):
                if at_end or (self.fmt == "%s" and len(v) > len(cache)):
                    m, _, ns, _ = Strptime(v[len(cache):], "%f", self.now)
                    ok = m >= 0
                else:
                    ok = True
            else:
                m, sec, ns, ns_len = Strptime(v, self.fmt, self.now, self.year)
                if sec is not None:
                    tv_sec = sec
                ok = m >= 0
                if ok:
                    cache = v[:m - ns_len if ns_len > 0 else m]
                    tv_sec -= self.offset
            if not ok:
                self.alarms.append((0, text + " " + self.fmt))
                self.counters["out_failed"] += 1
                out.append((text, 1, None))
            elif tv_sec <= 0 or (self.discard and self.now - tv_sec > self.interval):
                self.alarms.append((1, "logTime: %d" % tv_sec))
                self.counters["discarded"] += 1
                self.counters["history_failure"] += 1
            else:
                self.counters["out_successful"] += 1
                out.append((text, tv_sec, ns))
        return out
