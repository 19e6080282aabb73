"""tests/helpers/json_model.py -- the Python model of the JSON walk and of ProcessEvent -- against what pins it: the hand-written
contract vectors (tests/golden/json_contract_vectors.json), the reference's unit-test cases read as data
(tests/golden/json_unittest_vectors.json) and CPython's json module as an independent grammar check on generated documents."""
import json

from helpers import json_cases as jc
from helpers import json_model as jm


def test_the_model_gives_the_contract_vectors_literal_expectations():
    cases = jc.contract_cases()
    assert len(cases) >= 120
    for case in cases:
        line = jc.expand(case["line"])
        status, members, errpos = jm.walk(line)
        assert status == jc.STATUS_NAMES[case["status"]], (case["name"], errpos)
        if case["status"] == "ok":
            want = [[jc.expand(k), t, jc.expand(v)] for k, t, v in case["members"]]
            assert jc.rendered(line, members) == want, case["name"]
        elif case["status"] == "fail":
            assert errpos == case["errpos"], case["name"]


def test_the_model_gives_what_the_reference_s_unit_test_states():
    doc = jc.unittest_doc()
    assert len(doc["cases"]) >= 18
    for case in doc["cases"]:
        model = jm.Processor(case["config"])
        events = [{k.encode("latin-1"): v.encode("latin-1") for k, v in ev.items()} for ev in case["in"]]
        got = [e for e in (model.process_event(ev) for ev in events) if e is not None]
        assert got == [{k.encode("latin-1"): v.encode("latin-1") for k, v in ev.items()} for ev in case["expect"]], case["name"]
        c = {"discarded_events_total": model.counters["discarded"], "out_failed_events_total": model.counters["out_failed"],
             "in_events_total": len(events), "out_events_total": len(got)}
        for name, value in case["counters"].items():
            assert c[name] == value, (case["name"], name)
    for text in doc["invalid_formats"]:
        assert jm.walk(jc.expand(text))[0] == jm.FAIL, text


class _Obj(list):
    pass


def _cpython(doc, seen):
    """-> ('reject', None) or ('accept', value); seen: the constants CPython met"""
    try:
        text = doc.decode("utf-8", "strict")
        return "accept", json.loads(text, strict=True, object_pairs_hook=_Obj, parse_constant=lambda c: seen.append(c) or 0.0)
    except (UnicodeDecodeError, ValueError):
        return "reject", None


def _has_surrogate(v):
    if isinstance(v, str):
        return any(0xD800 <= ord(c) <= 0xDFFF for c in v)
    if isinstance(v, _Obj):
        return any(_has_surrogate(k) or _has_surrogate(x) for k, x in v)
    if isinstance(v, list):
        return any(_has_surrogate(x) for x in v)
    return False


def test_the_model_against_cpython_json_on_generated_documents_and_one_byte_mutations():
    docs = jc.generated_set(20261017, 21000)
    reasons = {"NaN / Infinity": 0, "lone surrogate escape": 0, "non-object root": 0, "depth beyond 1024": 0}
    both = rejected = 0
    for doc in docs:
        status, members, errpos = jm.walk(doc)
        seen = []
        verdict, value = _cpython(doc, seen)
        if verdict == "reject":
            assert status != jm.OK, ("the model accepts what CPython rejects", doc)
            rejected += 1
            continue
        if status != jm.OK:
            if seen:
                reasons["NaN / Infinity"] += 1
            elif not isinstance(value, _Obj):
                reasons["non-object root"] += 1
            elif _has_surrogate(value):
                reasons["lone surrogate escape"] += 1
            elif jm.max_depth_reached(doc) > jm.MAX_DEPTH:
                reasons["depth beyond 1024"] += 1
            else:
                raise AssertionError(("the model rejects what CPython accepts", doc, errpos))
            continue
        both += 1
        assert isinstance(value, _Obj) and len(value) == len(members), doc
        for (k, v), m in zip(value, members):
            key, text = jm.render(doc, m)
            assert key == k.encode("utf-8"), doc
            if isinstance(v, str):
                assert m.type == jm.STRING and text == v.encode("utf-8"), doc
            elif v is True or v is False or v is None:
                assert m.type == {True: jm.TRUE, False: jm.FALSE, None: jm.NULL}[v], doc
                assert text == {True: b"true", False: b"false", None: b""}[v], doc
            elif isinstance(v, int):
                fits = -(1 << 63) <= v < (1 << 64)
                assert m.type == (jm.INT if fits else jm.DOUBLE) and text == (b"%d" % v if fits else b"%f" % float(v)), doc
            elif isinstance(v, float):
                assert m.type == jm.DOUBLE and text == b"%f" % v, doc
            else:
                assert m.type == (jm.OBJECT if isinstance(v, _Obj) else jm.ARRAY) and text == doc[m.vb:m.ve], doc
                assert text[:1] + text[-1:] == (b"{}" if isinstance(v, _Obj) else b"[]"), doc
    assert len(docs) >= 20000 and both > 5000 and rejected > 5000, (both, rejected)
    assert reasons["NaN / Infinity"] and reasons["lone surrogate escape"] and reasons["non-object root"], reasons
    print("both accept %d, both reject %d, CPython alone accepts: %r" % (both, rejected, reasons))
