"""The pose fit (wave_pose, write_pose, kabsch_rotation, jacobi_pair — shared by k_pose, the stream solver's tail, k_small, the
multi-hypothesis rounds and k_ransac) against the mpmath truth of tests/golden/pose_truth.npz, at the edges of its own code: the
KEEP = 2 register window (k = 64, 65, 128, 129), clouds far from the origin, other length scales, nearly flat and nearly needle-shaped
clouds in general position, equal singular values, an exactly diagonal H, reflections, 2-D degenerate cases, k < dim inside a ragged
batch.  One roman_pose_batch call per dimension over the whole fixture; every assertion is against the truth, none against another
run of the device.  The bound K comes from the float64 reference's own error (tests/_pose_truth.py), not from the device."""
import numpy as np
import pytest

import _pose_truth as pt
from roman_amd import _abi

pytestmark = pytest.mark.gpu

CASES = pt.load()
BY_TAG = {c["tag"]: c for c in CASES}
DET = [c["tag"] for c in CASES if c["kind"] == pt.DETERMINED]
UNDET = [c["tag"] for c in CASES if c["kind"] == pt.UNDETERMINED]
SHORT = [c["tag"] for c in CASES if c["kind"] == pt.INSUFFICIENT]


@pytest.fixture(scope="module")
def fits(ctx):
    """tag -> (T, status): the two ragged batch calls (2-D, 3-D), made once."""
    out = {}
    for dim in (2, 3):
        idx, p1, p2, off = pt.batch(CASES, dim)
        T, status = ctx.pose_batch(dim, p1, p2, off)
        for j, i in enumerate(idx):
            out[CASES[i]["tag"]] = (T[j], int(status[j]))
    return out


def split(T, dim):
    assert np.array_equal(T[dim], np.eye(dim + 1)[dim])            # the last row of a rigid transform, exactly
    return T[:dim, :dim], T[:dim, dim]


def check_determined(c, T, status):
    R, t = split(T, c["dim"])
    eR, et = pt.determined_errors(c, R, t)
    orth, det = pt.properness(R)
    print(f"{c['tag']:26s} eR = {eR:9.3g}  et = {et:9.3g}  |R'R - I| = {orth:6.3g}  |det - 1| = {det:6.3g}  (units of 2^-52; K = {pt.K})")
    assert status == _abi.ROMAN_ST_OK
    assert eR <= pt.K and et <= pt.K, (c["tag"], eR, et)
    assert orth <= pt.K and det <= pt.K, (c["tag"], orth, det)
    return max(eR, et)


@pytest.mark.parametrize("tag", DET)
def test_determined_fit_is_within_K_of_the_truth(fits, tag):
    """|R - R*|_F <= K 2^-52 kappa (1 + c/r),  |t - t*| <= K 2^-52 kappa (1 + c/r) c,  R orthonormal with det +1 to K 2^-52, status 0."""
    check_determined(BY_TAG[tag], *fits[tag])


def test_largest_determined_error_is_reported(fits):
    """The device's own largest normalised error over the determined cases (DESIGN.md §2.2 quotes it): a report, the bound is K."""
    errs = []
    for tag in DET:
        c = BY_TAG[tag]
        R, t = split(fits[tag][0], c["dim"])
        errs.append((max(pt.determined_errors(c, R, t)), tag))
    worst = max(errs)
    print(f"device: largest normalised error {worst[0]:.2f} at {worst[1]}  (reference: {pt.REF_MAX}, K = {pt.K})")
    assert worst[0] <= pt.K


@pytest.mark.parametrize("tag", UNDET)
def test_undetermined_fit_is_proper_and_optimal(fits, tag):
    """Rank H <= 1 in 3-D: the turn about the line is free.  What is determined: a proper rotation, the optimal residual to
    K 2^-52 c sqrt(k), and the centroid of p2 mapped onto the centroid of p1 to the translation bound with kappa = 1.

    needle_h1e-09 is the case that found something.  Its cloud is 1 x 1e-9 x 5e-10: the exact optimum (residual 1.33e-11) aligns the
    1e-9 cross-section, but s2 / s1 = 7.6e-19 of H lies below the rounding of a float64 H (2^-53 s1), so a fit made from H alone turns
    the needle about its axis at random: in units of 2^-52 c sqrt(k) (bound: K = 64) the residual excess was 4.97e4 on the device and is
    3.4e5 for oracle.t_align (numpy).  wave_pose now takes a third sweep where it finds rank H <= 1: the cross-covariance of the
    points with their leading components taken out holds the cross-section, and its leading pair settles the turn (thin_rotation).
    needle_h1e-09_k129 / _k200 and collinear_k129 run that sweep past the 128-pair register window, where it fetches the points again."""
    c = BY_TAG[tag]
    T, status = fits[tag]
    R, t = split(T, c["dim"])
    orth, det = pt.properness(R)
    e_res, e_cen = pt.undetermined_errors(c, R, t)
    print(f"{tag:26s} residual excess = {e_res:9.3g}  centroid = {e_cen:9.3g}  |R'R - I| = {orth:6.3g}  |det - 1| = {det:6.3g}  (K = {pt.K})")
    assert status == _abi.ROMAN_ST_OK
    assert orth <= pt.K and det <= pt.K, (tag, orth, det)
    assert e_cen <= pt.K, (tag, e_cen)
    assert e_res <= pt.K, (tag, e_res)


@pytest.mark.parametrize("tag", SHORT)
def test_too_few_points_anywhere_in_the_batch(fits, tag):
    """k < dim — first, last and between the large cases of the ragged batch: INSUFFICIENT and an all-NaN pose.  (That the
    neighbours are untouched is what the other tests of this module assert on the same two calls.)"""
    T, status = fits[tag]
    assert status == _abi.ROMAN_ST_INSUFFICIENT and np.all(np.isnan(T)), tag


def test_single_problem_calls(ctx):
    """B = 1: the k = 129 case alone (one past the register window), and a lone k = 0."""
    c = BY_TAG["window_k129"]
    T, status = ctx.pose_batch(3, c["p1"], c["p2"], np.array([0, 129], dtype=np.int64))
    assert T.shape == (1, 4, 4)
    check_determined(c, T[0], int(status[0]))
    for dim in (2, 3):
        T, status = ctx.pose_batch(dim, np.zeros((0, dim)), np.zeros((0, dim)), np.array([0, 0], dtype=np.int64))
        assert T.shape == (1, dim + 1, dim + 1) and np.all(np.isnan(T))
        assert status.tolist() == [_abi.ROMAN_ST_INSUFFICIENT]
