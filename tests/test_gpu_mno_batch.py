"""roman_mno_batch: the reference's multi-solution loop [REF roman/align/object_registration.py:57-86] for a whole batch on the
device, against the same loop on the CPU oracle (tests/_mno_oracle.py: dense M and C of the scored pair, plain-CLIPPER solves,
the selected block of M zeroed in between), against the per-pair mno_clipper() on the same device, and at its edges.

Pass counts: every problem of these batches has at most ROMAN_MNO_MAX_ASSOC nodes and is served by the stream solver, whose
organisation of the passes the oracle reproduces in pass_mode("auto") — the mode tests/conftest.py gives every GPU test."""
import ctypes as C

import numpy as np
import pytest

from _mno_oracle import mno_from_dense, oracle_mno, plain_params, pose_of
from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import batch as rb
from roman_amd.runtime import Context, RomanHipError

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-5            # the value of tests/test_gpu_batch.py
SCORE_TOL = 1e-9           # the tolerance of tests/test_gpu_batch.py::test_dense_matrix_path_and_mno_clipper
K3 = 3

METHODS = {
    "roman": dict(semantics_dim=16), "semanticgrav": dict(semantics_dim=16), "gravity": {}, "clipper": {}, "clipper+prune": dict(cosine_min=0.5),
}
SIZES = [(14, 14), (40, 40), (30, 34), (19, 40), (40, 15), (25, 26), (33, 21)]      # 7 pairs per method: 35 in all, 14-40 objects per map


def _reg(method, ctx):
    reg = registration_for(method, **METHODS[method]); reg.set_context(ctx)
    return reg


def _pairs(method, seed0=300):
    d = 16 if method in ("roman", "semanticgrav", "clipper+prune") else 0
    out = []
    for k, (n, m) in enumerate(SIZES):
        pr = synth.make_pair(n, m, d, seed0 + k)
        out.append((pr.map1, pr.map2))
    return out


def _check_against_oracle(orc, reg, m1, m2, res, b, K, kmax=None, passes=True):
    """Solutions of problem b of `res` against the oracle's loop: arrays (order included), scores, pass counts, poses."""
    ref = oracle_mno(orc, reg, m1, m2, K)
    dim = reg.dim
    for k in range(K):
        full = ref[k]["assoc"]
        want = full if kmax is None else full[:kmax]
        print(f"  b={b} k={k}: {len(full)} associations, score {res.score[b, k]:.12f} (oracle {ref[k]['score']:.12f}), "
              f"passes {res.stats['n_pass'][b, k]} (oracle {ref[k]['stats'].n_pass}), status {res.status[b, k]}")
        assert np.array_equal(res.assoc[b][k].astype(np.int64), want), (b, k)
        assert abs(res.score[b, k] - ref[k]["score"]) < SCORE_TOL, (b, k)
        if passes and ref[k]["stats"].nnz_upper > 0:
            assert res.stats["n_pass"][b, k] == ref[k]["stats"].n_pass, (b, k)
        if kmax is not None and len(full) > kmax:
            assert res.status[b, k] & _abi.ROMAN_ST_ASSOC_TRUNCATED
        if len(full) >= dim:
            assert not (res.status[b, k] & _abi.ROMAN_ST_INSUFFICIENT)
            assert np.linalg.norm(res.T[b, k] - pose_of(orc, m1, m2, full, dim)) < POSE_TOL, (b, k)      # from the FULL set
        else:
            assert res.status[b, k] & _abi.ROMAN_ST_INSUFFICIENT and np.all(np.isnan(res.T[b, k])), (b, k)
    return ref


@pytest.mark.parametrize("method", list(METHODS))
def test_batch_equals_the_oracle_loop_and_poses(ctx, orc, method):
    """Checks 1 and 3: a ragged batch per method (35 pairs in all), K = 3: association arrays equal, scores within 1e-9,
    pass counts equal wherever nnz_upper > 0, poses within POSE_TOL of orc.t_align or the INSUFFICIENT bit and NaN."""
    reg = _reg(method, ctx)
    pairs = _pairs(method)
    res = rb.run_mno_batch(reg, rb.batch_from_pairs(reg, pairs), K3)
    assert res.score.shape == (len(pairs), K3) and res.T.shape == (len(pairs), K3, 4, 4)
    later = 0
    for b, (m1, m2) in enumerate(pairs):
        ref = _check_against_oracle(orc, reg, m1, m2, res, b, K3)
        later += sum(len(r["assoc"]) > 0 for r in ref[1:])
    assert later > 0                                   # the later rounds are short but not empty: masking and the tie path were exercised


@pytest.mark.parametrize("method", ["roman", "clipper", "clipper+prune"])
def test_batch_equals_per_pair_mno_clipper(ctx, method):
    """Check 2: mno_clipper_batch(pairs, K)[b] is mno_clipper(*pairs[b], K) — the dense, host-driven loop on the same device."""
    reg = _reg(method, ctx)
    pairs = _pairs(method, seed0=420)[:4]
    sols, poses = reg.mno_clipper_batch(pairs, num_solutions=K3)
    for b, (m1, m2) in enumerate(pairs):
        one = reg.mno_clipper(m1, m2, num_solutions=K3)
        assert len(sols[b]) == len(one) == K3
        for k in range(K3):
            assert sols[b][k][0].dtype == np.int64 and np.array_equal(sols[b][k][0], one[k][0]), (b, k)
            assert abs(sols[b][k][1] - one[k][1]) < SCORE_TOL, (b, k)


@pytest.mark.parametrize("method", ["clipper", "gravity"])
def test_solution_0_is_register_without_single_scores(ctx, method):
    """Check 4, first half: no single scores, so the plain-CLIPPER view is the scored problem itself."""
    reg = _reg(method, ctx)
    batch = rb.batch_from_pairs(reg, _pairs(method))
    res = rb.run_mno_batch(reg, batch, 2)
    base = rb.run_batch(reg, batch)
    for b in range(len(batch)):
        assert np.array_equal(res.assoc[b][0], base.assoc[b]), b
        assert np.allclose(res.T[b, 0], base.T[b], rtol=0, atol=1e-12, equal_nan=True)


def test_solution_0_of_roman_is_the_plain_solve_over_all_nodes(ctx, orc):
    """Check 4, second half: under the ROMAN invariant solution 0 solves over ALL A nodes with a unit diagonal — dead associations are
    isolated nodes — and is NOT register()'s array (30 x 34 objects, d = 32, seeds 5 and 6: checked with the oracle first)."""
    reg = _reg("roman", ctx); reg = registration_for("roman", semantics_dim=32); reg.set_context(ctx)
    pairs = [(pr.map1, pr.map2) for pr in (synth.make_pair(30, 34, 32, s) for s in (5, 6))]
    res = rb.run_mno_batch(reg, rb.batch_from_pairs(reg, pairs), K3)
    differs = 0
    for b, (m1, m2) in enumerate(pairs):
        ref = _check_against_oracle(orc, reg, m1, m2, res, b, K3)
        assert ref[0]["stats"].n_assoc_in == 30 * 34                       # every input association is a node of the oracle's solve
        assert res.stats["n_live"][b, 0] == 30 * 34
        o = orc.register(reg._abi_params(), reg.pack(m1), reg.pack(m2), None)
        assert not np.array_equal(ref[0]["assoc"], o["assoc"].astype(np.int64))       # the precondition, on the oracle
        r = reg.register(m1, m2)
        differs += not np.array_equal(res.assoc[b][0], r)
    assert differs >= 1


def test_masked_pairs_stay_consistent_pairs_of_weight_zero(ctx, orc):
    """Check 5: an explicit list (two thirds of the 12 x 12 all-to-all list, seed 923) whose SECOND solution differs between the two
    readings of the mask — M zeroed with C kept (the reference's) and the pair removed from C as well.  The device gives the first."""
    reg = _reg("clipper", ctx)
    pr = synth.make_pair(12, 12, 0, 923)
    A = orc.create_all_to_all(12, 12); A = np.ascontiguousarray(A[(A[:, 0] + 2 * A[:, 1]) % 3 != 0])
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    mat, _ = orc.build_matrix(reg._abi_params(), D1, D2, A)
    Mo, Co = mat.dense()
    kept = mno_from_dense(orc, plain_params(reg), Mo, Co, A, 2)
    removed = mno_from_dense(orc, plain_params(reg), Mo, Co, A, 2, mask_c=True)
    assert np.array_equal(kept[0]["assoc"], removed[0]["assoc"]) and not np.array_equal(kept[1]["assoc"], removed[1]["assoc"])   # precondition
    feats = np.concatenate([D1, D2])
    res = ctx.mno_batch(reg._abi_params(), feats, [0], [12], [12], [12], num_solutions=2, assoc=A, assoc_off=[0, len(A)], kmax=12)
    for k in range(2):
        assert np.array_equal(res.assoc[0][k].astype(np.int64), kept[k]["assoc"]), k
        assert abs(res.score[0, k] - kept[k]["score"]) < SCORE_TOL


def _aliased_pair(seed, n=12, noise=0.02):
    """Map 2 holds two copies of map 1's cluster under two rigid transforms (both map map-2 coordinates into map 1)."""
    rng = np.random.default_rng(seed)
    pts = synth._sample_centroids(rng, n, radius=6.0)
    Ta = synth.yaw_transform(0.4, np.array([3.0, -2.0, 0.1])); Tb = synth.yaw_transform(-1.1, np.array([-25.0, 30.0, -0.2]))
    seg = lambda i, c: synth.SyntheticSegment(i, c, 1.0, 0.5, 0.3, 0.2, np.ones(3), None)
    m1 = [seg(i, p) for i, p in enumerate(pts)]
    m2 = []
    for T in (Ta, Tb):
        Ti = np.linalg.inv(T)
        for p in pts:
            m2.append(seg(len(m2), Ti[:3, :3] @ p + Ti[:3, 3] + noise * rng.standard_normal(3)))
    return m1, m2, (Ta, Tb), pts, noise


def test_two_aisles_give_two_hypotheses(ctx, orc):
    """Check 6: perceptual aliasing.  Solutions 0 and 1 recover the two planted transforms: each hypothesis moves every point of
    its copy to within 5 sigma of the synthetic noise of where one planted transform puts it, and the two are distinct."""
    reg = _reg("clipper", ctx)
    cases = [_aliased_pair(s) for s in range(3)]

    def which(T, m2, planted, noise, copy_rows):
        x = np.array([m2[j].center.ravel()[:3] for j in copy_rows]); xh = np.c_[x, np.ones(len(x))]
        errs = [np.max(np.linalg.norm((xh @ T.T - xh @ P.T)[:, :3], axis=1)) for P in planted]
        k = int(np.argmin(errs))
        assert errs[k] < 5 * noise, errs
        return k

    for m1, m2, planted, pts, noise in cases:              # the precondition: the oracle's loop separates the two copies
        o = oracle_mno(orc, reg, m1, m2, 2)
        got = {which(pose_of(orc, m1, m2, s["assoc"]), m2, planted, noise, s["assoc"][:, 1]) for s in o}
        assert got == {0, 1}
    pairs = [(c[0], c[1]) for c in cases]
    sols, poses = reg.mno_clipper_batch(pairs, num_solutions=2)
    for (m1, m2, planted, pts, noise), s, T in zip(cases, sols, poses):
        assert len(s[0][0]) >= 8 and len(s[1][0]) >= 8
        got = {which(T[k], m2, planted, noise, s[k][0][:, 1]) for k in range(2)}
        assert got == {0, 1}
        assert np.linalg.norm(T[0] - T[1]) > 1.0


# ---- edges ------------------------------------------------------------------------------------------------------------------

def test_empty_maps_and_num_solutions_1(ctx, orc):
    reg = _reg("semanticgrav", ctx)
    pairs = []
    for k, (n, m) in enumerate([(20, 22), (0, 10), (10, 0), (16, 30)]):
        pr = synth.make_pair(max(n, 1), max(m, 1), 16, 510 + k)
        pairs.append((pr.map1[:n], pr.map2[:m]))
    batch = rb.batch_from_pairs(reg, pairs)
    for K in (1, 3):
        res = rb.run_mno_batch(reg, batch, K)
        assert res.score.shape == (4, K)
        for b, (m1, m2) in enumerate(pairs):
            if len(m1) == 0 or len(m2) == 0:
                for k in range(K):
                    assert res.status[b, k] & _abi.ROMAN_ST_EMPTY_MAP and res.assoc[b][k].shape == (0, 2)
                    assert res.score[b, k] == 0.0 and np.all(np.isnan(res.T[b, k]))
            else:
                _check_against_oracle(orc, reg, m1, m2, res, b, K)


def test_kmax_truncation_per_solution(ctx, orc):
    reg = _reg("clipper", ctx)
    pr = synth.make_pair(30, 30, 0, 1000)
    b = rb.batch_from_pairs(reg, [(pr.map1, pr.map2)])
    cut = ctx.mno_batch(reg._abi_params(), b.feats, b.off1, b.n1, b.off2, b.n2, num_solutions=2, kmax=5)
    ref = _check_against_oracle(orc, reg, pr.map1, pr.map2, cut, 0, 2, kmax=5)
    assert len(ref[0]["assoc"]) > 5 and cut.status[0, 0] & _abi.ROMAN_ST_ASSOC_TRUNCATED and len(cut.assoc[0][0]) == 5


def test_num_solutions_out_of_range_is_invalid(ctx):
    reg = _reg("clipper", ctx)
    pr = synth.make_pair(14, 14, 0, 33)
    b = rb.batch_from_pairs(reg, [(pr.map1, pr.map2)])
    for K in (0, -1, _abi.ROMAN_MNO_MAX_SOLUTIONS + 1):
        with pytest.raises(RomanHipError, match=r"\(-1\)"):
            ctx.mno_batch(reg._abi_params(), b.feats, b.off1, b.n1, b.off2, b.n2, num_solutions=K)
    big = synth.make_pair(60, 60, 0, 34)                    # 3600 associations: beyond the documented cap
    bb = rb.batch_from_pairs(reg, [(big.map1, big.map2)])
    with pytest.raises(RomanHipError, match=r"\(-6\)"):
        ctx.mno_batch(reg._abi_params(), bb.feats, bb.off1, bb.n1, bb.off2, bb.n2, num_solutions=2)
    P = reg._abi_params(); P.drift_aware = 1
    with pytest.raises(RomanHipError, match=r"\(-5\)"):
        ctx.mno_batch(P, b.feats, b.off1, b.n1, b.off2, b.n2, num_solutions=2)


def test_explicit_and_empty_lists_in_one_batch(ctx, orc):
    """An empty list means all-to-all, as in the batch call."""
    reg = _reg("clipper", ctx)
    prs = [synth.make_pair(16, 15, 0, 610 + k) for k in range(3)]
    lists = [None, None, None]
    A0 = orc.create_all_to_all(16, 15); lists[0] = np.ascontiguousarray(A0[::2]); lists[2] = np.ascontiguousarray(A0[1::3])
    feats = np.concatenate([reg.pack(m) for pr in prs for m in (pr.map1, pr.map2)])
    off1 = np.arange(3) * 31; off2 = off1 + 16
    assoc = np.concatenate([lists[0], lists[2]]); assoc_off = np.array([0, len(lists[0]), len(lists[0]), len(assoc)])
    res = ctx.mno_batch(reg._abi_params(), feats, off1, [16] * 3, off2, [15] * 3, num_solutions=2, assoc=assoc, assoc_off=assoc_off, kmax=15)
    P = plain_params(reg)
    for b, pr in enumerate(prs):
        mat, A = orc.build_matrix(reg._abi_params(), reg.pack(pr.map1), reg.pack(pr.map2), lists[b])
        Mo, Co = mat.dense()
        ref = mno_from_dense(orc, P, Mo, Co, A, 2)
        for k in range(2):
            assert np.array_equal(res.assoc[b][k].astype(np.int64), ref[k]["assoc"]) and abs(res.score[b, k] - ref[k]["score"]) < SCORE_TOL


_DEV_ENTRY = r"""
import os, sys
import numpy as np
import torch                                   # (torch owns the device memory: imported first, in a process of its own)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from _mno_oracle import mno_from_dense, plain_params
from oracle import oracle as orc
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams, batch as rb
from roman_amd.runtime import Context
orc.build()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
reg = SubmapAlignParams(method="gravity").get_object_registration()
c = Context(0, stream=stream.cuda_stream); reg.set_context(c)
batches = [rb.batch_from_pairs(reg, [(pr.map1, pr.map2) for pr in (synth.make_pair(20 + k, 24, 0, 640 + 10 * q + k) for k in range(3))]) for q in range(3)]
K, kmax = 2, 24
sol_dt = np.dtype([("n_assoc", np.int32), ("status", np.int32), ("score", np.float64), ("T", np.float64, (16,))])
assert sol_dt.itemsize == _abi.MNO_SOLUTION_NBYTES
feats = [torch.from_numpy(b.feats).to(dev) for b in batches]
a_out = [torch.zeros((3, K, kmax, 2), dtype=torch.int32, device=dev) for _ in batches]
s_out = [torch.zeros(3 * K * sol_dt.itemsize, dtype=torch.uint8, device=dev) for _ in batches]
st_out = [torch.zeros(3 * K * _abi.STATS_NBYTES, dtype=torch.uint8, device=dev) for _ in batches]
torch.cuda.synchronize(dev)
c.set_pipeline(3)
P = reg._abi_params()
todo = [np.arange(3) for _ in batches]
for attempt in range(5):
    for q, b in enumerate(batches):            # three calls in flight, one per batch; a skipped problem is issued again on its own
        if len(todo[q]) == 3:
            c.mno_batch_dev(P, feats[q].data_ptr(), b.feats.shape[1], b.off1, b.n1, b.off2, b.n2, K, kmax,
                            a_out[q].data_ptr(), s_out[q].data_ptr(), st_out[q].data_ptr())
        else:
            for i in todo[q]:
                c.mno_batch_dev(P, feats[q].data_ptr(), b.feats.shape[1], b.off1[i:i + 1], b.n1[i:i + 1], b.off2[i:i + 1], b.n2[i:i + 1], K, kmax,
                                a_out[q][i].data_ptr(), s_out[q].data_ptr() + int(i) * K * sol_dt.itemsize, st_out[q].data_ptr() + int(i) * K * _abi.STATS_NBYTES)
    c.sync()
    sols = [s.cpu().numpy().view(sol_dt).reshape(3, K) for s in s_out]
    for s in sols:                             # a skipped problem says so on EVERY solution
        assert np.all((s["status"][:, 0] & _abi.ROMAN_ST_WORKSPACE) == (s["status"][:, 1] & _abi.ROMAN_ST_WORKSPACE))
    todo = [np.nonzero(s["status"][:, 0] & _abi.ROMAN_ST_WORKSPACE)[0] for s in sols]
    print("attempt", attempt, "skipped", [len(t) for t in todo])
    if not any(len(t) for t in todo):
        break
assert not any(len(t) for t in todo)
c.set_pipeline(1)
with orc.pass_mode("auto"):
    for q, b in enumerate(batches):
        ao = a_out[q].cpu().numpy()
        stt = st_out[q].cpu().numpy().view(np.dtype([("n_assoc_in", np.int32), ("n_live", np.int32), ("nnz_upper", np.int64), ("n_pass", np.int32), ("outer_iters", np.int32),
                                                     ("inner_iters", np.int32), ("ls_trials", np.int32), ("score", np.float64), ("d_final", np.float64)])).reshape(3, K)
        for i in range(3):
            D1 = b.feats[b.off1[i]:b.off1[i] + b.n1[i]]; D2 = b.feats[b.off2[i]:b.off2[i] + b.n2[i]]
            mat, A = orc.build_matrix(P, D1, D2, None)
            Mo, Co = mat.dense()
            ref = mno_from_dense(orc, plain_params(reg), Mo, Co, A, K)
            for k in range(K):
                n = sols[q]["n_assoc"][i, k]
                assert np.array_equal(ao[i, k, :n].astype(np.int64), ref[k]["assoc"]), (q, i, k)
                assert abs(sols[q]["score"][i, k] - ref[k]["score"]) < 1e-9, (q, i, k)
                if ref[k]["stats"].nnz_upper > 0:
                    assert stt["n_pass"][i, k] == ref[k]["stats"].n_pass, (q, i, k)
c.close()
print("device-pointer entry: ok")
"""


def test_device_pointer_entry_at_pipeline_depth_3():
    """roman_mno_batch_dev on device memory, three calls in flight, then roman_ctx_sync; skipped problems carry ROMAN_ST_WORKSPACE on
    every solution and are issued again; every problem against the oracle's loop."""
    import subprocess, sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _DEV_ENTRY], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0 and "device-pointer entry: ok" in r.stdout


def test_host_entry_chunks_a_large_batch(orc):
    """B above the host-batching chunk with small maps: calls of `chunk` problems, three in flight, re-issues; a sample against the oracle."""
    reg = registration_for("roman", semantics_dim=16)
    c = Context(0)
    try:
        reg.set_context(c)
        c.set_host_batching(64, 3)
        subs, _ = synth.make_submap_grid(26, n=14, d=16, seed0=900)
        batch = rb.batch_from_submap_grid(reg, subs[:13], subs[13:])
        assert len(batch) == 169 > 64
        res = rb.run_mno_batch(reg, batch, 2)
        assert not np.any(res.status & (_abi.ROMAN_ST_WORKSPACE | _abi.ROMAN_ST_INTERNAL))
        for b in (0, 63, 64, 100, 168):
            i, j = batch.pair_index[b]
            _check_against_oracle(orc, reg, subs[i], subs[13 + j], res, b, 2)
    finally:
        c.close()
