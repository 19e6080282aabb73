"""Writes tests/golden/timestamp_strptime_vectors.json: the output of the REFERENCE's OWN strptime_ns for (format, value) pairs.

    python tests/golden/gen_timestamp_vectors.py          (needs the reference tree; CPU only)

No test, build() or smoke() runs this.  core/common/Strptime.cpp is compiled as it stands into a temporary directory, next to a small
driver that calls strptime_ns the way Strptime() of core/common/TimeUtil.cpp does (struct tm zeroed, tm_year = INT_MIN, nanosecondLength
= -1) and prints the return value, the fields, the nanoseconds and glibc's mktime of the fields.  The driver runs once per TZ setting
(POSIX strings: no zoneinfo files are needed).  Only the JSON is kept.

This is the FLOOR tier of README_timestamp.md; the processor-level tier (ProcessorParseTimestampNative.cpp compiled from source) was
not reached, see there.
"""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LC_REFERENCE_CORE", "/root/reference/core")
OUT = os.path.join(ROOT, "tests", "golden", "timestamp_strptime_vectors.json")
TZS = ["UTC", "CST-8", "EST5EDT,M3.2.0,M11.1.0"]

DRIVER = r'''
#include <climits>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <strings.h>
#include "common/Strptime.h"
namespace logtail { int CStringNCaseInsensitiveCmp(const char* a, const char* b, size_t n) { return strncasecmp(a, b, n); } }
static std::string unhex(const std::string& h) {
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back(char(std::stoi(h.substr(i, 2), nullptr, 16)));
    return s;
}
int main() {
    tzset();
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t tab = line.find('\t');
        const std::string fmt = unhex(line.substr(0, tab)), val = unhex(line.substr(tab + 1));
        struct tm tm;
        memset(&tm, 0, sizeof tm);
        tm.tm_year = INT_MIN;
        long ns = 0;
        int nsLen = -1;
        const char* r = logtail::strptime_ns(val.c_str(), fmt.c_str(), &tm, &ns, &nsLen);
        struct tm copy = tm;
        const long long t = (long long)mktime(&copy);
        printf("%ld %d %d %d %d %d %d %d %ld %d %lld\n", r ? long(r - val.c_str()) : -1L, tm.tm_sec, tm.tm_min, tm.tm_hour, tm.tm_mday,
               tm.tm_mon, tm.tm_year, tm.tm_isdst, ns, nsLen, t);
    }
    return 0;
}
'''

# (format, [values]): the reference's unit test and example configs, every conversion once, names in mixed case, one- and two-digit
# fields, out-of-range fields, trailing bytes, empty and short values, %f in the middle and at the end, %s with 10 / 13 / 16 / 19
# digits, %z in each of its forms, formats without a year, prefix collisions
CASES = [
    ("%Y-%m-%d %H:%M:%S", ["2023-12-25 01:02:03", "2012-01-01 15:05:07", "2024-02-29 23:59:59", "2023-02-29 00:00:00", "2023-13-01 00:00:00",
                           "2023-12-32 00:00:00", "2023-1-2 3:4:5", "2023-12-25 24:00:00", "2023-12-25 23:60:00", "2023-12-25 23:59:60",
                           "2023-12-25 23:59:61", "2023-12-25 23:59:62", "", "2023", "2023-12-25", "2023-12-25 01:02:03trailing",
                           "2023-12-25 01:02:03+08:00", "0000-01-01 00:00:00", "9999-12-31 23:59:59", "1969-12-31 23:59:59",
                           "1970-01-01 00:00:00", "2023-04-31 12:00:00", "2023-11-05 01:30:00", "2023-03-12 02:30:00", "2023-03-12 03:30:00",
                           "2023-07-01 12:00:00", "x", "2023-12-25  01:02:03", "2023-12-25\t\n01:02:03", "12345-01-01 00:00:00",
                           "1900-01-01 00:00:00", "2100-02-29 00:00:00", "2000-02-29 00:00:00", "0001-01-01 00:00:00"]),
    ("%Y-%m-%d %H:%M:%S.%f", ["2023-12-25 01:02:03.123", "2023-12-25 01:02:03.123456", "2023-12-25 01:02:03.123456789",
                              "2023-12-25 01:02:03.1234567890", "2023-12-25 01:02:03.12345678901234", "2023-12-25 01:02:03.",
                              "2023-12-25 01:02:03.5 tail", "2023-12-25 01:02:03.000000001", "2023-12-25 01:02:03"]),
    ("%Y-%m-%d %H:%M:%S.%f %z", ["2023-12-25 01:02:03.123 +0800", "2023-12-25 01:02:03.123456 Z", "2023-12-25 01:02:03.1+08"]),
    ("%f %H:%M", ["123 10:15", "999999999 23:59", "x 10:15"]),
    ("%H:%M:%S,%f", ["10:15:20,123", "10:15:20,1", "10:15:2,55"]),
    ("%d/%b/%Y:%H:%M:%S %z", ["25/Dec/2023:01:02:03 +0800", "25/dec/2023:01:02:03 -0500", "25/DEC/2023:01:02:03 +08:00",
                              "5/Jan/2023:1:2:3 +08", "25/December/2023:01:02:03 Z", "25/Dece/2023:01:02:03 Z", "25/Dec/2023:01:02:03 GMT",
                              "25/Dec/2023:01:02:03 UT", "25/Dec/2023:01:02:03 EST", "25/Dec/2023:01:02:03 EDT", "25/Jul/2023:01:02:03 PDT",
                              "25/Dec/2023:01:02:03 cst", "25/Dec/2023:01:02:03 A", "25/Dec/2023:01:02:03 J", "25/Dec/2023:01:02:03 M",
                              "25/Dec/2023:01:02:03 Y", "25/Dec/2023:01:02:03 +0860", "25/Dec/2023:01:02:03 +08:", "25/Dec/2023:01:02:03 +8",
                              "25/Dec/2023:01:02:03 +080", "25/Dec/2023:01:02:03 GX", "25/Dec/2023:01:02:03 UX", "25/Dec/2023:01:02:03",
                              "25/Dec/2023:01:02:03    +0800", "25/Dec/2023:01:02:03 +0800x", "25/Xyz/2023:01:02:03 +0800",
                              "25/Dec/2023:01:02:03 +08::30", "25/Dec/2023:01:02:03 e"]),
    ("%Y-%m-%dT%H:%M:%S%Z", ["2023-12-25T01:02:03GMT", "2023-12-25T01:02:03utc", "2023-12-25T01:02:03CST", "2023-12-25T01:02:03"]),
    ("%s", ["1700000000", "1700000000123", "1700000000123456", "1700000000123456789", "17000000001234567890123", "12345", "0", "",
            "abc", " 1700000000", "+1700000000", "-5", "1700000000 tail", "1700000000.5", "0000000001700000000", "99999999999999999999999",
            "-17000000001", "17e3"]),
    ("%s.%f", ["1700000000.5"]),
    ("%b %d %H:%M:%S", ["Dec 25 01:02:03", "Feb 29 12:00:00", "Jan  1 00:00:00", "Dec 31 23:59:59", "Jan 1 00:00:00", "Feb 30 00:00:00",
                        "Apr 31 00:00:00", "dEc 5 1:2:3", "May 10 10:10:10", "Mar 12 02:30:00", "Nov 5 01:30:00"]),
    ("%H:%M", ["10:1", "10:15", "10:15:20", "1:5", "24:00", "9", ""]),
    ("%H:%M:%S", ["00:00:00", "23:59:59"]),
    ("%A %a %B %b %h", ["Monday mon January jan feb", "SUNDAY Sat MARCH May may", "Mon Monday Jan January Dec", "Mond mon January jan feb",
                        "Wednesday wed September sep oct"]),
    ("%C%y-%m-%d", ["2023-12-25", "1999-01-01", "0523-01-01"]),
    ("%y%C", ["2320", "6919", "0000"]),
    ("%y-%m-%d", ["23-12-25", "68-01-01", "69-01-01", "99-12-31", "00-01-01", "5-1-1", "x"]),
    ("%C", ["20", "0", "99", "x"]),
    ("%C %C", ["19 20"]),
    ("%y %y", ["23 45"]),
    ("%D %T", ["12/25/23 01:02:03", "12/25/69 01:02:03", "1/2/3 4:5:6"]),
    ("%F %R", ["2023-12-25 01:02", "2023-12-25 01:02:03"]),
    ("%f %T", ["123 01:02:03"]),
    ("%T.%f", ["01:02:03.25"]),
    ("%C %D", ["19 12/25/23"]),
    ("%Y %r", ["2023 01:02:03 PM", "2023 12:02:03 AM", "2023 12:02:03 pm", "2023 11:59:59 am", "2023 13:02:03 PM", "2023 00:02:03 PM",
               "2023 01:02:03 XM", "2023 01:02:03"]),
    ("%Y %I %p", ["2023 12 AM", "2023 12 PM", "2023 1 pm"]),
    ("%Y %H %p", ["2023 13 PM", "2023 11 PM", "2023 11 AM"]),
    ("%Y %l %k", ["2023 11 23", "2023 0 23"]),
    ("%c", ["Mon Dec 25 01:02:03 2023", "mon dec  5 1:2:3 2023", "Mon Dec 25 01:02:03"]),
    ("%x %X", ["12/25/23 01:02:03"]),
    ("%Ec %EC %Ex %EX %EY", ["Mon Dec 25 01:02:03 2023 20 12/25/23 01:02:03 2023"]),
    ("%Od %Oe %OH %OI %Om %OM %OS %OU %Ow %OW %Ou %Oy %Of", ["25 25 13 1 12 59 59 52 1 52 1 23 5"]),
    ("%Ed", ["25"]), ("%OY", ["2023"]), ("%EOd", ["25"]), ("%OEd", ["25"]), ("%Ek", ["12"]), ("%Ol", ["12"]), ("%OD", ["12/25/23"]),
    ("%Oc", ["Mon Dec 25 01:02:03 2023"]), ("%E%", ["%"]), ("%%Y%Y", ["%Y2023", "Y2023"]), ("%Ea", ["Mon"]), ("%Ep", ["AM"]),
    ("%Ej", ["100"]), ("%En", [" "]), ("%Eg %EG %EV %Ey %EZ %Ez", ["23 2023 52 23 GMT Z"]),
    ("%Y %j %U %W %u %w %g %G %V", ["2023 359 52 52 1 1 23 2023 52", "2023 366 53 53 7 6 99 20234 53", "2023 367 1 1 1 1 1 1 1",
                                    "2023 0 1 1 1 1 1 1 1", "2023 1 54 1 1 1 1 1 1", "2023 1 1 1 8 1 1 1 1", "2023 1 1 1 0 1 1 1 1",
                                    "2023 1 1 1 1 7 1 1 1", "2023 1 1 1 1 1 1 x 1"]),
    ("%Y%n%m%t%d", ["2023 12 25", "20231225", "2023\t\t12\n25"]),
    ("%Y%m%d%H%M%S", ["20231225010203", "2023122501020", "202312250102035"]),
    ("%Y %q", ["2023 x"]), ("%Y %", ["2023 "]), ("%Y %E", ["2023 "]), ("%Y %s", ["2023 1700000000"]),
    ("time=%H", ["time=10", "tame=10", "time=", "tim"]),
    ("%m/%d/%Y", ["2/30/2023", "12/31/2023", "1/0/2023", "0/1/2023"]),
    ("%d %m", ["31 12", "1 1", "31 4", "29 2"]),
    ("[%Y-%m-%d %H:%M:%S]", ["[2023-12-25 01:02:03]", "[2023-12-25 01:02:03", "2023-12-25 01:02:03]"]),
    # the formats and values of ProcessorParseTimestampNativeUnittest.cpp (TestParseLogTime, TestParseLogTimeSecondCache,
    # TestAdjustTimeZone, TestProcessNoYearFormat)
    ("[%Y-%m-%d %H:%M:%S.%f", ["[2017-1-11 15:05:07.0123]"]),
    ("%d %b %y %H:%M", ["11 Jan 17 15:05 MST", "11 Jan 17 15:05 -0700"]),
    ("%A, %d-%b-%y %H:%M:%S.%f", ["Tuesday, 11-Jan-17 15:05:07.0123 MST"]),
    ("%A, %d %b %Y %H:%M:%S", ["Tuesday, 11 Jan 2017 15:05:07 MST"]),
    ("%Y-%m-%dT%H:%M:%S", ["2017-01-11T15:05:07Z08:00"]),
    ("%Y-%m-%dT%H:%M:%S.%f", ["2017-01-11T15:05:07.012999999Z07:00", "2026-03-09T14:39:49.985+08:00"]),
    ("%H:%M:%S.%f %Y-%m-%d", ["15:05:07.012 2017-1-11", "15:05:00.0 2012-01-01", "15:05:04.4 2012-01-01", "15:04:59.0 2012-01-01"]),
    ("%Y-%m-%d %H:%M:%S.%f %z (%Z)", ["2017-1-11 15:05:07.012 +0700 (UTC)"]),
    ("%m-%d %H:%M:%S.%f", ["12-25 10:26:40.999999999", "02-29 00:00:00.999999999"]),
    ("%s", ["1484147107", "1484147107123", "1484147106", "14841471070", "14841471114"]),
    ("%Y-%m-%d %H:%M:%S", ["2017-1-11 15:05:07.012", "2012-01-01 15:04:59", "2012-01-01 15:05:00", "2012-01-01 15:05:04"]),
    ("%Y-%m-%d %H:%M:%S.%f", ["2017-1-11 15:05:07.012", "2012-01-01 15:05:00.0", "2012-01-01 15:05:04.4"]),
    ("%Y-%m-%d %H:%M:%S %z", ["2023-12-25 01:02:03 EDT", "2023-07-04 12:00:00 EDT", "2023-03-12 02:30:00 EDT", "2023-11-05 01:30:00 EDT",
                              "2023-11-05 01:30:00 EST"]),
]


def random_cases(rng):
    out = []
    fmts = ["%Y-%m-%d %H:%M:%S", "%d/%b/%Y:%H:%M:%S %z", "%b %d %H:%M:%S", "%Y-%m-%dT%H:%M:%S.%f", "%s", "%y%m%d %I:%M:%S %p", "%c"]
    months = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]
    days = ["Sun", "Mon", "Tue", "Wed", "Thu", "Fri", "Sat"]
    for fmt in fmts:
        vals = []
        for _ in range(40):
            y, mo, d = rng.choice([1970, 1999, 2000, 2023, 2024, 2038, 2100, rng.randrange(0, 10000)]), rng.randrange(1, 13), rng.randrange(1, 32)
            h, mi, s = rng.randrange(0, 24), rng.randrange(0, 60), rng.randrange(0, 62)
            v = {"%Y-%m-%d %H:%M:%S": "%04d-%02d-%02d %02d:%02d:%02d" % (y, mo, d, h, mi, s),
                 "%d/%b/%Y:%H:%M:%S %z": "%02d/%s/%04d:%02d:%02d:%02d %s" % (d, months[mo - 1], y, h, mi, s, rng.choice(["+0800", "-0330", "Z", "EDT", "+05:45"])),
                 "%b %d %H:%M:%S": "%s %2d %02d:%02d:%02d" % (months[mo - 1], d, h, mi, s),
                 "%Y-%m-%dT%H:%M:%S.%f": "%04d-%02d-%02dT%02d:%02d:%02d.%s" % (y, mo, d, h, mi, s, str(rng.randrange(10 ** rng.randrange(1, 10)))),
                 "%s": str(rng.randrange(10 ** rng.randrange(1, 20))),
                 "%y%m%d %I:%M:%S %p": "%02d%02d%02d %02d:%02d:%02d %s" % (y % 100, mo, d, h % 12 + 1, mi, s, rng.choice(["AM", "pm", "Pm"])),
                 "%c": "%s %s %2d %02d:%02d:%02d %d" % (rng.choice(days), months[mo - 1], d, h, mi, s, y)}[fmt]
            if rng.random() < 0.15:  # damage one byte
                k = rng.randrange(len(v))
                v = v[:k] + rng.choice("x:/ 9-") + v[k + 1:]
            vals.append(v)
        out.append((fmt, vals))
    return out


def main():
    pairs = []
    for fmt, vals in CASES + random_cases(random.Random(20240917)):
        for v in vals:
            pairs.append((fmt, v))
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cpp")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-include", "set", "-include", "memory", "-include", "string",
                               "-I", os.path.join(ROOT, "oracle", "ref_processor", "stubs"), "-I", os.path.join(ROOT, "oracle", "ref_models", "stubs"),
                               "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF,
                               "-I", os.path.join(REF, "config"), "-o", exe, drv, os.path.join(REF, "common", "Strptime.cpp")])
        text = "".join("%s\t%s\n" % (f.encode("latin-1").hex(), v.encode("latin-1").hex()) for f, v in pairs)
        per_tz = {}
        for tz in TZS:
            env = dict(os.environ, TZ=tz)
            res = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, env=env, check=True).stdout.decode().splitlines()
            assert len(res) == len(pairs)
            per_tz[tz] = [[int(x) for x in line.split()] for line in res]
    vectors = []
    for i, (fmt, val) in enumerate(pairs):
        rows = [per_tz[tz][i] for tz in TZS]
        base = rows[0]
        rec = {"format": fmt, "value": val, "matched": base[0], "nanos": base[8], "nanos_len": base[9],
               "mktime": {tz: per_tz[tz][i][10] for tz in TZS}}
        if fmt == "%s":  # localtime_r fills the fields: they differ per zone, mktime gives the second back
            rec["tm"] = None
        else:
            assert all(r[:10] == base[:10] for r in rows), (fmt, val)
            rec["tm"] = dict(zip(["sec", "min", "hour", "mday", "mon", "year", "isdst"], base[1:8]))
        vectors.append(rec)
    with open(OUT, "w") as f:
        json.dump({"tz": TZS, "vectors": vectors}, f, separators=(",", ":"), ensure_ascii=True)
    print("%s: %d vectors, %d bytes" % (OUT, len(vectors), os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())
