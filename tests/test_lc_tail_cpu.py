"""The NumPy statement of the loop-closure tail (tests/_lc_tail.py) against the EXISTING per-pair code — submap_align()
pass 2, loop_closure_edges(), transform_to_xyz_quat() — on planted transforms: rotations beside gimbal lock, roll / pitch on
both sides of 90 degrees and of the 5 degree tilt threshold, NaN poses with every failure status, dim 2, association counts
at thresh - 1 / thresh / thresh + 1, a pair the time gate disables (see make_cases)."""
import numpy as np
import pytest

import _lc_tail as lt
from roman_amd import _abi
from roman_amd.runtime import LcInputs


@pytest.mark.parametrize("kw", lt.ALL_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_numpy_tail_matches_the_per_pair_code(kw):
    case = lt.make_cases(**kw)
    want, want_acc = lt.host_reference_in_tail_terms(case)
    got, got_acc = lt.lc_tail(lt.lc_inputs(case), case["T"], case["n_assoc"], case["status"])
    lt.assert_records_match(got, got_acc, want, want_acc, abs_theta=True)
    # the cases really contain what they claim
    f = want["flags"]
    assert np.any(f & _abi.ROMAN_LC_FAILED_INSUFFICIENT) and np.any(f & _abi.ROMAN_LC_ACCEPTED)
    k = case["thresh_idx"]
    assert [int(x & _abi.ROMAN_LC_ACCEPTED) for x in f[k:k + 3]] == [0, 1, 1] and not np.any(f[k:k + 3] & _abi.ROMAN_LC_FAILED)   # thresh - 1 / thresh / thresh + 1
    assert not (f[-1] & _abi.ROMAN_LC_ACCEPTED) and want["n_assoc"][-1] >= lt.THRESH                                  # the time gate
    if case["dim"] == 3 and case["upside_down"] and not case["tilt"]:
        assert np.any(f & _abi.ROMAN_LC_FAILED_UPSIDE_DOWN)
    if case["tilt"]:
        assert np.any(f & _abi.ROMAN_LC_FAILED_TILT)
    assert np.all(np.diff(got_acc) > 0)


def test_statuses_without_a_result_are_flagged_not_failed():
    """ROMAN_ST_WORKSPACE / ROMAN_ST_INTERNAL: neither failed nor accepted, sentinels, whatever the count says."""
    T = np.tile(np.eye(4), (4, 1, 1)); T[1:3] = np.nan
    rec, acc = lt.lc_tail(LcInputs(lc_association_thresh=1, T_ref=T.copy() * 0 + np.eye(4)), T, [5, 5, 5, 0],
                          [0, _abi.ROMAN_ST_WORKSPACE, _abi.ROMAN_ST_INTERNAL, 0])
    assert rec["flags"].tolist() == [_abi.ROMAN_LC_ACCEPTED, _abi.ROMAN_LC_SKIPPED, _abi.ROMAN_LC_INTERNAL, 0]
    assert acc.tolist() == [0] and rec["n_assoc"].tolist() == [5, 0, 0, 0]
    assert np.all(np.isnan(rec["T_hat"][1:3])) and rec["theta"][1:3].tolist() == [180.0, 180.0] and rec["dist"][1:3].tolist() == [1e6, 1e6]
    assert rec["theta"][0] == 0.0 and rec["dist"][0] == 0.0 and np.array_equal(rec["edge_q"][0], [0, 0, 0, 1.0])


def test_quaternion_sign_is_scipys():
    """as_quat() is not canonicalised: rotations whose w comes out negative keep it."""
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(11)
    R = Rot.random(500, random_state=7).as_matrix()
    R = np.concatenate([R, Rot.from_euler('z', [np.pi - 1e-9, -np.pi + 1e-9, 3.0, -3.0]).as_matrix()])
    q = lt.quat_from_matrix(R)
    want = np.stack([Rot.from_matrix(r).as_quat() for r in R])
    np.testing.assert_allclose(q, want, rtol=0, atol=1e-12)
    assert np.any(q[:, 3] < 0)
