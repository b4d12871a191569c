"""roman_mno_lc_tail_dev (k_mno_lc_tail + both compactions) alone, over planted roman_mno_solution_t arrays.

Per (b, k) the kernel must be k_lc_tail's arithmetic: its records are compared BITWISE with roman_lc_tail_dev on the same device
over the flattened B*K poses with the per-problem inputs repeated K times, and within the project's tolerances with the NumPy
statement (tests/_mno_lc.py).  The best hypothesis and both lists are pure functions of the records and must equal the host
statement exactly.  The planted poses are those of tests/_lc_tail.make_cases (beside 90 degrees, beside the tilt threshold, beside
gimbal lock, every status), dealt over the (problem, hypothesis) grid."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _lc_tail as lt
import _mno_lc as ml
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import LcInputs, RomanHipError, lc_record_dtype, mno_solution_dtype
from test_gpu_lc_tail import device_tail

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 64), (5, 3), (257, 2), (65, 64)]
UNTOUCHED = -7


def device_mno_tail(ctx, lc, sol):
    """Upload, roman_mno_lc_tail_dev, download -> (records (B*K,), best, accepted, accepted_best); the slots of both lists beyond
    their counts must come back as uploaded."""
    B, K = sol.shape
    T_ref, enable, FL, iL, FR, iR = lc.arrays(B)
    hip = Hip()
    try:
        up = lambda a: None if a is None else hip.upload(a)
        d_rec = hip.alloc(B * K * _abi.LC_RECORD_NBYTES)
        d_best = hip.upload(np.full(B, UNTOUCHED, np.int32))
        d_idx = hip.upload(np.full(B * K, UNTOUCHED, np.int32)); d_cnt = hip.upload(np.array([UNTOUCHED], np.int32))
        d_bidx = hip.upload(np.full(B, UNTOUCHED, np.int32)); d_bcnt = hip.upload(np.array([UNTOUCHED], np.int32))
        ctx.mno_lc_tail_dev(lc.params(), B, K, hip.upload(sol), d_rec, d_best, d_idx, d_cnt, d_bidx, d_bcnt,
                            T_ref_ptr=up(T_ref), enable_ptr=up(enable), FL_ptr=up(FL), iL_ptr=up(iL), FR_ptr=up(FR), iR_ptr=up(iR))
        ctx.sync()
        cnt = int(hip.download(d_cnt, (1,), np.int32)[0]); bcnt = int(hip.download(d_bcnt, (1,), np.int32)[0])
        assert 0 <= cnt <= B * K and 0 <= bcnt <= B
        idx = hip.download(d_idx, (B * K,), np.int32); bidx = hip.download(d_bidx, (B,), np.int32)
        assert np.all(idx[cnt:] == UNTOUCHED) and np.all(bidx[bcnt:] == UNTOUCHED)
        return hip.download(d_rec, (B * K,), lc_record_dtype()), hip.download(d_best, (B,), np.int32), idx[:cnt], bidx[:bcnt]
    finally:
        hip.free_all()


def planted(B, K, dim, seed, tilt=False, **switches):
    """-> (lc with B-entry arrays, sol (B, K)): make_cases' poses dealt over the grid in order, its per-pair inputs over the problems."""
    case = lt.make_cases(dim=dim, seed=seed, tilt=tilt, **switches)
    full = lt.lc_inputs(case)
    Bc = case["B"]
    p = np.arange(B * K) % Bc; q = (np.arange(B) * 7) % Bc
    sol = np.zeros((B, K), dtype=mno_solution_dtype())
    s = sol.reshape(-1)
    s["n_assoc"] = case["n_assoc"][p]; s["status"] = case["status"][p]; s["score"] = 1.0
    s["T"][:, :(dim + 1) ** 2] = case["T"][p].reshape(B * K, -1)
    lc = dataclasses.replace(full, T_ref=np.asarray(full.T_ref)[q], enable=np.asarray(full.enable)[q], iL=np.asarray(full.iL)[q], iR=np.asarray(full.iR)[q])
    return lc, sol


def poses(sol, dim):
    B, K = sol.shape
    return sol["T"][:, :, :(dim + 1) ** 2].reshape(B, K, dim + 1, dim + 1)


def check(ctx, lc, sol):
    B, K = sol.shape
    got, best, acc, acc_best = device_mno_tail(ctx, lc, sol)
    # the same arithmetic as k_lc_tail, to the bit
    flat, flat_acc = device_tail(ctx, ml.repeated(lc, K), poses(sol, lc.dim).reshape(B * K, lc.dim + 1, lc.dim + 1), sol["n_assoc"].reshape(-1), sol["status"].reshape(-1))
    assert got.tobytes() == flat.tobytes()
    np.testing.assert_array_equal(acc, flat_acc)
    # the host statement
    want, want_best, want_acc, want_acc_best = ml.mno_lc_tail(lc, K, poses(sol, lc.dim), sol["n_assoc"], sol["status"])
    lt.assert_records_match(got, acc, want, want_acc)
    np.testing.assert_array_equal(got["problem"], np.arange(B * K))
    np.testing.assert_array_equal(best, want_best)
    np.testing.assert_array_equal(best, ml.best_rule(got, B, K))          # a pure function of the records
    np.testing.assert_array_equal(acc_best, want_acc_best)
    return got, best, acc, acc_best


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("B, K", SHAPES)
def test_records_best_and_lists(ctx, B, K, dim):
    lc, sol = planted(B, K, dim, seed=B + K, tilt=(B % 2 == 1 and dim == 3))
    got, best, acc, acc_best = check(ctx, lc, sol)
    if B * K >= 64:                                                          # the planted set holds every kind of record
        assert np.any(got["flags"] & _abi.ROMAN_LC_ACCEPTED) and np.any(got["flags"] & _abi.ROMAN_LC_FAILED_INSUFFICIENT)
        if dim == 3:
            assert np.any(got["flags"] & (_abi.ROMAN_LC_FAILED_UPSIDE_DOWN | _abi.ROMAN_LC_FAILED_TILT))


def test_without_optional_inputs_and_repeatable(ctx):
    """NULL T_ref / enable / FL / FR; two runs are bitwise equal."""
    lc, sol = planted(65, 3, 3, seed=11)
    bare = LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=lt.THRESH)
    a = check(ctx, bare, sol)
    assert np.all(np.isnan(a[0]["theta"][(a[0]["flags"] & ~_abi.ROMAN_LC_ACCEPTED) == 0]))      # no reference transform: no error metric
    b = device_mno_tail(ctx, bare, sol)
    assert a[0].tobytes() == b[0].tobytes()
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
    only_left = dataclasses.replace(lc, FR=None, iR=None, T_ref=None)
    check(ctx, only_left, sol)


def test_best_rule_cases(ctx):
    """Hypothesis 0 upside down with a valid hypothesis 1; equal counts; all failed; a skipped problem; a disabled problem whose
    best exists but is not accepted; a best below the association threshold."""
    K = 3
    ok = np.eye(4); ok[:3, :3] = lt.sa_rot(0.7, 0.01, -0.02); ok[:3, 3] = (1.0, -2.0, 0.5)
    flipped = np.eye(4); flipped[:3, :3] = lt.sa_rot(-1.1, 0.02, np.pi - 0.3)           # roll beyond 90 degrees
    nan = np.full((4, 4), np.nan)
    W, INS = _abi.ROMAN_ST_WORKSPACE, _abi.ROMAN_ST_INSUFFICIENT
    rows = [                                                                            # (pose, n_assoc, status) per hypothesis; expected best
        ([(flipped, 20, 0), (ok, 10, 0), (ok, 6, 0)], 1),
        ([(ok, 8, 0), (ok, 8, 0), (ok, 8, 0)], 0),
        ([(ok, 5, 0), (ok, 8, 0), (ok, 8, 0)], 1),
        ([(nan, 0, INS), (flipped, 9, 0), (nan, 2, INS)], -1),
        ([(nan, 0, W), (nan, 0, W), (nan, 0, W)], -1),
        ([(ok, 7, 0), (ok, 12, 0), (flipped, 30, 0)], 1),                               # enable == 0 below
        ([(ok, 1, 0), (ok, 3, 0), (ok, 2, 0)], 1),                                      # all below lc_association_thresh
        ([(nan, 0, INS), (nan, 0, INS), (ok, 4, 0)], 2),
    ]
    B = len(rows)
    sol = np.zeros((B, K), dtype=mno_solution_dtype())
    for b, (hyps, _) in enumerate(rows):
        for k, (T, n, st) in enumerate(hyps):
            sol[b, k]["T"] = T.ravel(); sol[b, k]["n_assoc"] = n; sol[b, k]["status"] = st
    enable = np.ones(B, np.int32); enable[5] = 0
    lc = LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=lt.THRESH,
                  T_ref=np.tile(np.eye(4), (B, 1, 1)), enable=enable)
    got, best, acc, acc_best = check(ctx, lc, sol)
    np.testing.assert_array_equal(best, [r[1] for r in rows])
    flags = got["flags"].reshape(B, K)
    assert flags[0, 0] == _abi.ROMAN_LC_FAILED_UPSIDE_DOWN and flags[0, 1] & _abi.ROMAN_LC_ACCEPTED
    assert np.all(flags[4] == _abi.ROMAN_LC_SKIPPED)
    assert np.all(flags[5] & _abi.ROMAN_LC_ACCEPTED == 0) and np.all(flags[6] == 0)
    np.testing.assert_array_equal(acc_best, [0, 1, 2, 7])
    np.testing.assert_array_equal(acc, [1, 2, 3, 4, 5, 6, 7, 8, 23])


def test_refusals_and_empty_batch(ctx):
    """ROMAN_E_INVALID with text and nothing enqueued; B == 0 sets both counts to 0."""
    lp = LcInputs(dim=3).params()
    hip = Hip()
    try:
        buf = hip.upload(np.full(64, UNTOUCHED, np.int32))
        def refused(B, K, sol=buf, rec=buf, best=buf, text=""):
            with pytest.raises(RomanHipError, match=text) as e:
                ctx.mno_lc_tail_dev(lp, B, K, sol, rec, best, buf, buf, buf, buf)
            assert e.value.code == _abi.ROMAN_E_INVALID
        refused(-1, 2, text="B < 0")
        refused(1, 0, text="num_solutions"); refused(1, _abi.ROMAN_MNO_MAX_SOLUTIONS + 1, text="num_solutions")
        refused(1, 2, sol=None, text="sol"); refused(1, 2, rec=None, text="records"); refused(1, 2, best=None, text="best")
        bad = LcInputs(dim=4).params()
        with pytest.raises(RomanHipError, match="dim"):
            ctx.mno_lc_tail_dev(bad, 1, 2, buf, buf, buf, buf, buf, buf, buf)
        ctx.sync()
        assert np.all(hip.download(buf, (64,), np.int32) == UNTOUCHED)               # nothing ran
        c1 = hip.upload(np.array([UNTOUCHED], np.int32)); c2 = hip.upload(np.array([UNTOUCHED], np.int32))
        ctx.mno_lc_tail_dev(lp, 0, 2, None, None, None, None, c1, None, c2)
        ctx.sync()
        assert hip.download(c1, (1,), np.int32)[0] == 0 and hip.download(c2, (1,), np.int32)[0] == 0
    finally:
        hip.free_all()


def test_the_other_refusals(ctx):
    """B * K above INT32_MAX, a frame pool without its index array, NULL counts, lc_params.dim against params.point_dim in the
    fused call, and the frame indices the host-pointer call can check: ROMAN_E_INVALID, nothing enqueued."""
    from roman_amd import synth
    from roman_amd.align import batch as rb
    from conftest import registration_for
    lp = LcInputs(dim=3).params()
    hip = Hip()
    try:
        buf = hip.upload(np.full(64, UNTOUCHED, np.int32))
        def refused(text, *a, **kw):
            with pytest.raises(RomanHipError, match=text) as e:
                ctx.mno_lc_tail_dev(*a, **kw)
            assert e.value.code == _abi.ROMAN_E_INVALID
        refused("int32", lp, 1 << 26, 64, buf, buf, buf, buf, buf, buf, buf)
        refused("come together", lp, 1, 2, buf, buf, buf, buf, buf, buf, buf, FL_ptr=buf)
        refused("come together", lp, 1, 2, buf, buf, buf, buf, buf, buf, buf, iR_ptr=buf)
        refused("n_accepted", lp, 1, 2, buf, buf, buf, buf, None, buf, buf)
        refused("n_accepted", lp, 1, 2, buf, buf, buf, buf, buf, buf, None)
        reg = registration_for("gravity"); reg.set_context(ctx)
        pr = synth.make_pair(8, 8, 0, 3)
        batch = rb.batch_from_pairs(reg, [(pr.map1, pr.map2)])
        with pytest.raises(RomanHipError, match="point_dim") as e:
            ctx.mno_lc_batch_dev(reg._abi_params(), buf, 3, batch.off1, batch.n1, batch.off2, batch.n2, 2, 8, buf, buf, LcInputs(dim=2).params(),
                                 buf, buf, buf, buf, buf, buf)
        assert e.value.code == _abi.ROMAN_E_INVALID
        frames = np.tile(np.eye(4), (2, 1, 1))
        for kw, text in ((dict(FL=frames, iL=[2]), "iL"), (dict(FR=frames, iR=[-1]), "iR")):
            with pytest.raises(RomanHipError, match=text) as e:
                rb.run_mno_lc_batch(reg, batch, LcInputs(dim=3, **kw), 2)
            assert e.value.code == _abi.ROMAN_E_INVALID
        ctx.sync()
        assert np.all(hip.download(buf, (64,), np.int32) == UNTOUCHED)               # nothing ran
    finally:
        hip.free_all()
