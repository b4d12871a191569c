"""roman_lc_tail_dev (k_lc_tail + k_lc_compact) against the NumPy statement of the tail (tests/_lc_tail.py) on the planted
cases of tests/test_lc_tail_cpu.py, uploaded as they are: flags, counts, the accepted list and its order identical, floats
within the project's tolerances for the same quantities.  Before anything goes to the device the cases are decided on the CPU
by the NumPy statement AND by the per-pair scipy code, which must agree (every planted angle keeps 1e-6 rad from a threshold,
where a decision would hang on atan2's last bits)."""
import numpy as np
import pytest

import _lc_tail as lt
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import LcInputs, lc_record_dtype

pytestmark = pytest.mark.gpu


def device_tail(ctx, lc, T, n_assoc, status):
    """Upload, roman_lc_tail_dev, download -> (records, accepted)."""
    status = np.ascontiguousarray(status, dtype=np.int32); B = status.shape[0]
    T16 = np.zeros((B, 16)); flat = np.asarray(T, dtype=np.float64).reshape(B, (lc.dim + 1) ** 2); T16[:, :flat.shape[1]] = flat
    T_ref, enable, FL, iL, FR, iR = lc.arrays(B)
    hip = Hip()
    try:
        up = lambda a: None if a is None else hip.upload(a)
        d_rec = hip.alloc(B * _abi.LC_RECORD_NBYTES); d_idx = hip.alloc(B * 4); d_cnt = hip.upload(np.array([-7], np.int32))
        ctx.lc_tail_dev(lc.params(), B, hip.upload(T16), hip.upload(np.ascontiguousarray(n_assoc, dtype=np.int32)), hip.upload(status),
                        d_rec, d_idx, d_cnt, T_ref_ptr=up(T_ref), enable_ptr=up(enable), FL_ptr=up(FL), iL_ptr=up(iL), FR_ptr=up(FR), iR_ptr=up(iR))
        ctx.sync()
        cnt = int(hip.download(d_cnt, (1,), np.int32)[0])
        assert 0 <= cnt <= B
        return hip.download(d_rec, (B,), lc_record_dtype()), hip.download(d_idx, (B,), np.int32)[:cnt]
    finally:
        hip.free_all()


@pytest.mark.parametrize("kw", lt.ALL_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_device_tail_matches_numpy_statement(ctx, kw):
    case = lt.make_cases(**kw)
    lc = lt.lc_inputs(case)
    want, want_acc = lt.lc_tail(lc, case["T"], case["n_assoc"], case["status"])
    host, host_acc = lt.host_reference_in_tail_terms(case)      # the per-pair scipy code decides every case alike ...
    np.testing.assert_array_equal(host["flags"], want["flags"]); np.testing.assert_array_equal(host_acc, want_acc)
    got, got_acc = device_tail(ctx, lc, case["T"], case["n_assoc"], case["status"])           # ... before the device sees them
    lt.assert_records_match(got, got_acc, want, want_acc)       # every case of the batch is compared
    assert np.all(got["reserved"] == 0)


def test_statuses_without_a_result(ctx):
    """ROMAN_ST_WORKSPACE / ROMAN_ST_INTERNAL records: flagged, sentinels, never accepted; optional inputs absent."""
    case = lt.make_cases(dim=3, seed=9)
    st = case["status"].copy(); st[3] = _abi.ROMAN_ST_WORKSPACE; st[4] = _abi.ROMAN_ST_INTERNAL; st[5] = _abi.ROMAN_ST_WORKSPACE | _abi.ROMAN_ST_INSUFFICIENT
    lc = LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=lt.THRESH)    # no T_ref, no enable, no frames
    want, want_acc = lt.lc_tail(lc, case["T"], case["n_assoc"], st)
    got, got_acc = device_tail(ctx, lc, case["T"], case["n_assoc"], st)
    lt.assert_records_match(got, got_acc, want, want_acc)
    assert got["flags"][3] == _abi.ROMAN_LC_SKIPPED and got["flags"][4] == _abi.ROMAN_LC_INTERNAL and got["flags"][5] == _abi.ROMAN_LC_SKIPPED
    ok = (got["flags"] & ~_abi.ROMAN_LC_ACCEPTED) == 0
    assert np.all(np.isnan(got["theta"][ok])) and np.all(np.isnan(got["dist"][ok]))          # no reference transform: no error metrics


@pytest.mark.parametrize("B, mode", [(0, "mixed"), (1, "all"), (1, "none"), (5000, "mixed"), (5000, "all"), (5000, "none"), (1025, "mixed")])
def test_compaction_sizes(ctx, B, mode):
    """B = 0, 1 and 5000 (several problems per thread of the scan's workgroup), all accepted, none accepted: the accepted list is
    the ascending list of the accepted problems."""
    rng = np.random.default_rng(B + len(mode))
    from scipy.spatial.transform import Rotation as Rot
    T = np.tile(np.eye(4), (B, 1, 1))
    if B:
        T[:, :3, :3] = Rot.from_euler('ZYX', np.stack([rng.uniform(-3, 3, B), rng.normal(0, 0.02, B), rng.normal(0, 0.02, B)], axis=1)).as_matrix()
        T[:, :3, 3] = rng.uniform(-5, 5, (B, 3))
    n = {"all": np.full(B, 9), "none": np.full(B, 1), "mixed": rng.integers(0, 9, B)}[mode].astype(np.int32)
    status = np.zeros(B, np.int32)
    lc = LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=lt.THRESH, T_ref=T.copy(),
                  enable=None if mode != "mixed" else (rng.uniform(size=B) < 0.7).astype(np.int32))
    want, want_acc = lt.lc_tail(lc, T, n, status)
    got, got_acc = device_tail(ctx, lc, T, n, status)
    lt.assert_records_match(got, got_acc, want, want_acc)
    assert len(got_acc) == {"all": B, "none": 0}.get(mode, len(want_acc))
