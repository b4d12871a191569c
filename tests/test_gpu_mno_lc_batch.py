"""roman_mno_lc_batch_dev / roman_mno_lc_batch: the K solves of roman_mno_batch with the hypothesis tail behind them.  8 problems
of 5-40 objects, d = 16, K = 3: the fused device call equals roman_mno_batch_dev followed by roman_mno_lc_tail_dev bitwise, the
host-pointer entry equals both, and all agree with the oracle's mno loop (tests/_mno_oracle.py) followed by the host statement of
the tail (tests/_mno_lc.py): identical association arrays, flags and best, poses within the bound of tests/test_gpu_mno_batch.py."""
import numpy as np
import pytest

import _lc_tail as lt
import _mno_lc as ml
from _hipmem import Hip
from _mno_oracle import oracle_mno, pose_of
from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import batch as rb
from roman_amd.runtime import LcInputs, lc_record_dtype, mno_solution_dtype
from test_gpu_mno_batch import POSE_TOL

pytestmark = pytest.mark.gpu
K = 3
SIZES = [(5, 9), (40, 40), (12, 30), (33, 21), (8, 8), (25, 26), (40, 15), (19, 37)]


@pytest.fixture(scope="module")
def problem():
    reg = registration_for("semanticgrav", semantics_dim=16)
    pairs = []
    for k, (n, m) in enumerate(SIZES):
        pr = synth.make_pair(n, m, 16, 700 + k)
        pairs.append((pr.map1, pr.map2))
    B = len(pairs)
    rng = np.random.default_rng(5)
    frames = np.tile(np.eye(4), (4, 1, 1))
    for f in frames:
        f[:3, :3] = lt.sa_rot(rng.uniform(-3, 3), rng.normal(0, 0.05), rng.normal(0, 0.05)); f[:3, 3] = rng.uniform(-3, 3, 3)
    T_ref = np.tile(np.eye(4), (B, 1, 1))
    for T in T_ref:
        T[:3, :3] = lt.sa_rot(rng.uniform(-3, 3), 0.0, 0.0); T[:3, 3] = rng.uniform(-5, 5, 3)
    enable = np.ones(B, np.int32); enable[1] = 0
    lc = LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=lt.THRESH, T_ref=T_ref, enable=enable,
                  FL=frames, iL=np.arange(B) % 4, FR=frames[::-1].copy(), iR=(np.arange(B) * 3) % 4)
    return reg, pairs, lc


def _device_forms(ctx, reg, batch, lc):
    """-> [(sol, assoc, records, best, acc, acc_best)] of the fused call and of mno_batch_dev + mno_lc_tail_dev."""
    B, kmax, P = len(batch), batch.kmax(), reg._abi_params()
    F = batch.feats.shape[1]
    T_ref, enable, FL, iL, FR, iR = lc.arrays(B)
    out = []
    hip = Hip()
    try:
        d_feats = hip.upload(batch.feats)
        d_assoc = None if batch.assoc is None else hip.upload(batch.assoc)
        opt = dict(T_ref_ptr=hip.upload(T_ref), enable_ptr=hip.upload(enable), FL_ptr=hip.upload(FL), iL_ptr=hip.upload(iL), FR_ptr=hip.upload(FR), iR_ptr=hip.upload(iR))
        for fused in (True, False):
            d_a = hip.upload(np.full((B, K, kmax, 2), -1, np.int32)); d_sol = hip.alloc(B * K * _abi.MNO_SOLUTION_NBYTES)
            d_rec = hip.alloc(B * K * _abi.LC_RECORD_NBYTES); d_best = hip.upload(np.full(B, -7, np.int32))
            d_idx = hip.upload(np.full(B * K, -7, np.int32)); d_cnt = hip.upload(np.array([-7], np.int32))
            d_bidx = hip.upload(np.full(B, -7, np.int32)); d_bcnt = hip.upload(np.array([-7], np.int32))
            if fused:
                ctx.mno_lc_batch_dev(P, d_feats, F, batch.off1, batch.n1, batch.off2, batch.n2, K, kmax, d_a, d_sol, lc.params(),
                                     d_rec, d_best, d_idx, d_cnt, d_bidx, d_bcnt, assoc_ptr=d_assoc, assoc_off=batch.assoc_off, **opt)
            else:
                ctx.mno_batch_dev(P, d_feats, F, batch.off1, batch.n1, batch.off2, batch.n2, K, kmax, d_a, d_sol, assoc_ptr=d_assoc, assoc_off=batch.assoc_off)
                ctx.join()
                ctx.mno_lc_tail_dev(lc.params(), B, K, d_sol, d_rec, d_best, d_idx, d_cnt, d_bidx, d_bcnt, **opt)
            ctx.sync()
            cnt = int(hip.download(d_cnt, (1,), np.int32)[0]); bcnt = int(hip.download(d_bcnt, (1,), np.int32)[0])
            out.append((hip.download(d_sol, (B, K), mno_solution_dtype()), hip.download(d_a, (B, K, kmax, 2), np.int32),
                        hip.download(d_rec, (B, K), lc_record_dtype()), hip.download(d_best, (B,), np.int32),
                        hip.download(d_idx, (B * K,), np.int32)[:cnt], hip.download(d_bidx, (B,), np.int32)[:bcnt]))
    finally:
        hip.free_all()
    return out


def test_fused_call_host_call_and_oracle(ctx, orc, problem):
    reg, pairs, lc = problem
    reg.set_context(ctx)
    batch = rb.batch_from_pairs(reg, pairs)
    B = len(batch)
    fused, split = _device_forms(ctx, reg, batch, lc)
    assert not np.any(fused[0]["status"] & _abi.ROMAN_ST_WORKSPACE)
    for a, b in zip(fused, split):                                   # the fused call IS the two calls
        assert a.tobytes() == b.tobytes()
    host = rb.run_mno_lc_batch(reg, batch, lc, K)
    sol, assoc, rec, best, acc, acc_best = fused
    assert host.records.tobytes() == rec.tobytes()
    np.testing.assert_array_equal(host.best, best); np.testing.assert_array_equal(host.accepted, acc); np.testing.assert_array_equal(host.accepted_best, acc_best)
    np.testing.assert_array_equal(host.n_assoc, sol["n_assoc"]); np.testing.assert_array_equal(host.status, sol["status"])
    assert host.T.tobytes() == sol["T"].reshape(B, K, 4, 4).tobytes()
    for b in range(B):
        for k in range(K):
            np.testing.assert_array_equal(host.assoc[b][k], assoc[b, k, :sol["n_assoc"][b, k]])
    # the oracle's loop, its poses, the host statement of the tail
    T = np.full((B, K, 4, 4), np.nan); n = np.zeros((B, K), np.int32); st = np.zeros((B, K), np.int32)
    for b, (m1, m2) in enumerate(pairs):
        for k, s in enumerate(oracle_mno(orc, reg, m1, m2, K)):
            np.testing.assert_array_equal(host.assoc[b][k].astype(np.int64), s["assoc"])
            n[b, k] = len(s["assoc"])
            if n[b, k] >= 3:
                T[b, k] = pose_of(orc, m1, m2, s["assoc"])
                assert np.linalg.norm(host.T[b, k] - T[b, k]) < POSE_TOL, (b, k)
            else:
                st[b, k] = _abi.ROMAN_ST_INSUFFICIENT
    want, want_best, want_acc, want_acc_best = ml.mno_lc_tail(lc, K, T, n, st)
    got = host.records.reshape(-1)
    print("flags", got["flags"].reshape(B, K).tolist(), "n_assoc", got["n_assoc"].reshape(B, K).tolist(), "best", best.tolist())
    np.testing.assert_array_equal(got["flags"], want["flags"]); np.testing.assert_array_equal(got["n_assoc"], want["n_assoc"])
    np.testing.assert_array_equal(best, want_best); np.testing.assert_array_equal(acc, want_acc); np.testing.assert_array_equal(acc_best, want_acc_best)
    np.testing.assert_allclose(got["T_hat"], want["T_hat"], rtol=0, atol=POSE_TOL, equal_nan=True)
    assert len(acc_best) >= 1 and np.all(got["flags"].reshape(B, K)[1] & _abi.ROMAN_LC_ACCEPTED == 0)      # the disabled problem has no edge
    assert 1 not in acc_best and best[1] >= 0
