"""The batch wrappers of roman_amd.runtime.Context against tests/golden/runtime_calls_golden.json, without a GPU: for every case
of tests/_runtime_calls.py the arguments that reach the C ABI (decoded by the recording library of that module), the result the
wrapper unpacks from the pattern the recorder writes, the exception it raises, what it does to Context._generation, and the
signatures of the 18 methods.  The golden file was written by tests/golden/make_runtime_calls_golden.py from the runtime.py of the
commit named in its "generated_from", before the wrappers were folded onto shared helpers; this module holds the tree to it field
by field.  One difference is on purpose: the host outputs of roman_align_batch_resident are compared as the wrapper returns them,
not as they are handed in (tests/_runtime_calls.UNDEFINED_ON_ENTRY)."""
import json
import os

import pytest

import _runtime_calls as rc
from conftest import GOLDEN
from roman_amd import _abi

with open(os.path.join(GOLDEN, "runtime_calls_golden.json")) as f:
    GOLD = json.load(f)


@pytest.fixture(scope="module")
def now():
    """Every case run once against this tree (the recorder stands behind _abi only while they run)."""
    before = _abi._LIB
    _abi._LIB = rc.CallRecorder()
    try:
        return json.loads(json.dumps(rc.run_all()))                # through JSON like the stored one: tuples, key types
    finally:
        _abi._LIB = before


def differences(want, got, path=""):
    """Paths at which two JSON values differ."""
    if isinstance(want, dict) and isinstance(got, dict):
        out = [f"{path}/{k}: only in the {'golden' if k in want else 'tree'}" for k in sorted(set(want) ^ set(got))]
        return out + [d for k in sorted(set(want) & set(got)) for d in differences(want[k], got[k], f"{path}/{k}")]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for i, (w, g) in enumerate(zip(want, got)) for d in differences(w, g, f"{path}[{i}]")]
    if type(want) is type(got) and want == got:
        return []
    return [f"{path}: golden {str(want)[:120]!r}, tree {str(got)[:120]!r}"]


def test_the_cases_are_the_goldens_cases(now):
    assert sorted(now["cases"]) == sorted(GOLD["cases"]) == sorted(rc.CASE_IDS)
    assert "generated_from" in GOLD


@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_case_matches_the_golden_transcript(now, cid):
    want, got = GOLD["cases"][cid], now["cases"][cid]
    for field in ("method", "rc", "outcome", "calls", "generation_delta", "transcript", "result", "exception", "counts_is_the_callers",
                  "callers_counts_after"):
        assert (field in want) == (field in got), field
        if field in want:
            diff = differences(want[field], got[field], field)
            assert not diff, "\n".join(diff[:20])
    assert set(want) == set(got)


def test_signatures_are_the_goldens(now):
    assert sorted(now["signatures"]) == sorted(rc.METHODS)
    for m in rc.METHODS:
        assert now["signatures"][m] == GOLD["signatures"][m], m


def test_every_method_ran_at_rc_0_and_at_an_error(now):
    """No method of the table drops out silently: at least one rc = 0 case that returned and one library error, per method."""
    for m in rc.METHODS:
        mine = [c for c in now["cases"].values() if c["method"] == m]
        assert any(c["rc"] == 0 and c["outcome"] == "returned" for c in mine), m
        assert any(c["rc"] != 0 and c["outcome"] == "raised" and c["exception"]["type"] == "RomanHipError" for c in mine), m
        reached = [c for c in mine if c["outcome"] == "returned" or c["exception"]["type"] == "RomanHipError"]
        assert all(c["calls"] == ["roman_" + m] for c in reached), m          # one library call each, the method's own entry


def test_a_value_error_precedes_the_call(now):
    bad = [c for c in now["cases"].values() if c["outcome"] == "raised" and c["exception"]["type"] == "ValueError"]
    assert len(bad) == 18
    for c in bad:
        assert c["calls"] == [] and c["transcript"] == [] and c["generation_delta"] == 0


def test_return_codes(now):
    """0: the result.  ROMAN_E_INTERNAL: a RomanHipError that carries the rc = 0 result for exactly the four host-result calls of
    the align family.  Any other code: err.code and the entry's name in the message."""
    for cid, c in now["cases"].items():
        if cid.endswith("-internal"):
            e, m = c["exception"], c["method"]
            assert c["rc"] == _abi.ROMAN_E_INTERNAL and e["type"] == "RomanHipError"
            assert e["message"] == f"roman_{m} failed ({_abi.ROMAN_E_INTERNAL}): {rc.LAST_ERROR.decode()}"
            assert e["has_result"] == (m in rc.CARRIES_RESULT), m
            assert e["result"] == ({"same_as": cid[:-len("-internal")]} if m in rc.CARRIES_RESULT else None), m
            assert c["transcript"] == {"same_as": cid[:-len("-internal")]}
        elif cid.endswith("-toolarge"):
            e, m = c["exception"], c["method"]
            assert e["type"] == "RomanHipError" and e["code"] == _abi.ROMAN_E_TOO_LARGE and not e["has_result"] and e["result"] is None
            assert e["message"] == f"roman_{m} failed ({_abi.ROMAN_E_TOO_LARGE}): {rc.LAST_ERROR.decode()}"
            assert c["transcript"] == {"same_as": cid[:-len("-toolarge")]}
    assert sorted({c["method"] for cid, c in now["cases"].items() if cid.endswith("-internal")}) == sorted(rc.METHODS)


def test_which_calls_bump_the_generation(now):
    """The calls that take workspace 0 (where the stepwise problem lives) bump Context._generation once, library error or not; the
    pure enqueues of the RANSAC, shared-ids and tail entries do not (the comment on Context._generation says why)."""
    quiet = {"lc_tail_dev", "mno_lc_tail_dev", "ransac_batch_dev", "ransac_lc_batch_dev", "shared_ids_dev", "shared_reduce_dev"}
    for cid, c in now["cases"].items():
        called = bool(c["calls"])
        assert c["generation_delta"] == int(called and c["method"] not in quiet), cid


def test_a_callers_counts_array_comes_back_itself(now):
    c = now["cases"]["ransac_batch/B2-kmax-own-counts"]
    assert c["counts_is_the_callers"] is True and c["callers_counts_after"]["values"] == list(range(50, 58))
    assert now["cases"]["ransac_lc_batch/B2-kmax-own-counts"]["callers_counts_after"]["values"] == list(range(50, 58))


def test_what_the_tail_receives(now):
    """NULL and counts of the optional tail inputs, as the cases name them."""
    def args(cid):
        return dict(now["cases"][cid]["transcript"][0]["args"])
    a = args("align_lc_batch/B2")
    assert [a[k] for k in ("T_ref", "enable", "FL", "iL", "FR", "iR")] == [None] * 6 and (a["n_left"], a["n_right"]) == (0, 0)
    a = args("align_lc_batch/B2-ref")
    assert a["T_ref"]["shape"] == [32] and a["enable"]["values"] == [0, 1] and a["FL"] is None and (a["n_left"], a["n_right"]) == (0, 0)
    a = args("align_lc_batch/B3-left")
    assert a["FL"]["shape"] == [48] and a["iL"]["values"] == [0, 1, 2] and a["FR"] is None and (a["n_left"], a["n_right"]) == (3, 0)
    for cid in ("align_lc_batch/B3-both", "align_lc_batch_ids/B3-no-keep", "ransac_lc_batch/B3-both-counts"):
        a = args(cid)
        assert (a["n_left"], a["n_right"]) == (3, 2) and a["FR"]["shape"] == [32] and a["iR"]["values"] == [0, 1, 0], cid
    assert args("align_lc_batch_ids/B3-no-keep")["keep"] is None and args("align_lc_batch_ids/B2")["keep"]["every"] == -1
    assert args("ransac_lc_batch_dev/B2-no-tail")["lc_params"] is None and args("ransac_lc_batch_dev/B3-all")["lc_params"]["struct"] == "RomanLcParams"
    assert args("mno_batch/B2-K0")["sol_out"]["shape"] == [0] and now["cases"]["mno_batch/B2-K0"]["result"]["fields"][1][1]["shape"] == [2, 0]
