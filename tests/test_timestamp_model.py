"""The Python model of the timestamp processor (helpers/timestamp_model.py) against every floor vector of
tests/golden/timestamp_strptime_vectors.json: the reference's own strptime_ns (return value, fields, nanoseconds) and glibc's mktime of
those fields under each TZ setting.  The model is what the host and GPU suites compare random values and whole groups against."""
import json
import os
import time

import pytest

from helpers import timestamp_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "timestamp_strptime_vectors.json")) as _f:
    _GOLD = json.load(_f)


def test_model_equals_reference_strptime_ns():
    for v in _GOLD["vectors"]:
        matched, tm, ns, ns_len, epoch = model.strptime_ns(v["value"].encode("latin-1"), v["format"])
        where = (v["format"], v["value"])
        assert matched == v["matched"], where
        if v["tm"] is not None:
            assert tm == v["tm"], where
            assert ns == v["nanos"] % 2 ** 32 and ns_len == v["nanos_len"], where
        elif matched >= 0:
            assert ns == v["nanos"] % 2 ** 32 and ns_len == v["nanos_len"], where


@pytest.mark.parametrize("zone", _GOLD["tz"])
def test_model_mktime_equals_recorded(zone):
    old = os.environ.get("TZ")
    os.environ["TZ"] = zone
    time.tzset()
    try:
        for v in _GOLD["vectors"]:
            matched, sec, _, _ = model.Strptime(v["value"].encode("latin-1"), v["format"], 1700000000, -1)
            if v["tm"] is None and matched < 0:
                continue  # a failed "%s" leaves the zeroed fields: the recorded mktime is of those
            assert sec == v["mktime"][zone], (v["format"], v["value"], zone)
    finally:
        if old is None:
            os.environ.pop("TZ", None)
        else:
            os.environ["TZ"] = old
        time.tzset()
