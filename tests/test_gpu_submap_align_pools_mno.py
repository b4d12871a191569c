"""submap_align_pools / submap_align_session with num_solutions on the device, end to end over two small maps (cap 12, d = 16), K = 2:
against the stand-in run of the same call over host pools (tests/test_mno_lc_cpu.py ties that run to the per-pair oracle loop) under
the radius gate with mean_semantic, the bounding-box gate without a descriptor and a [pool, pool] self case; a session of three
robots against submap_align_pools per block; and, with method='gravity' (no single scores) and K = 1, against the existing
single-solution path on the same device.  Runs in a process of its own (torch and the library share the device there)."""
import copy
import subprocess
import sys

import numpy as np
import pytest

D = 16


def _build(method, descriptor, device, ctx, build_ctx=None):
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    reg = SubmapAlignParams(method=method, semantics_dim=D).get_object_registration(); reg.set_context(ctx)
    params = SubmapParams(max_size=12, radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor=descriptor)
    pools = []
    import _session as ss
    base = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
    for r in range(2):                                           # two views of one place, each with its own ids and centres a little off:
        sg, traj, times = ss.robot_view(*base, r, keep=1.0 - 0.15 * r)    # (two copies of one map make exact ties in u, whose order hangs on last bits)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=build_ctx or ctx, device=device))
    return reg, pools


def _same(got, want, tol):
    assert np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
    np.testing.assert_allclose(got.T_ij_hat_mat, want.T_ij_hat_mat, rtol=0, atol=tol, equal_nan=True)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
    n0, n1 = want.clipper_num_associations.shape
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j, np.asarray(got.associated_objs_mat[i][j]).tolist(), np.asarray(want.associated_objs_mat[i][j]).tolist())


def _same_hyps(got, want, tol):
    assert set(got.hypotheses) == set(want.hypotheses)
    for key, hyps in want.hypotheses.items():
        for a, b in zip(got.hypotheses[key], hyps):
            assert np.array_equal(a[0], b[0]) and a[3:5] == b[3:5] and (a[5] is None) == (b[5] is None), key
            np.testing.assert_allclose(a[2], b[2], rtol=0, atol=tol, equal_nan=True)


def run_all_on_the_device():
    import torch
    import _mno_lc as ml
    import _submaps_oracle as so
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    POSE = 1e-5                                                  # the pose bound of tests/test_gpu_mno_batch.py against the oracle

    def stand_in(method, descriptor, p, self_case=False):
        stub = ml.stub_context()
        reg, pools = _build(method, descriptor, "cpu", stub, so.OracleSubmapContext())
        stub.n_objects = 0
        return sa.submap_align_pools(p, [pools[0], pools[0]] if self_case else pools, io, registration=reg, num_solutions=2)

    cases = [("radius-mean_semantic", "roman", 'mean_semantic', dict(submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8), False),
             ("aabb", "gravity", None, dict(force_fill_submaps=True), False),
             ("self", "gravity", None, dict(single_robot_lc=True, single_robot_lc_time_thresh=40.0), True)]
    for name, method, descriptor, kw, self_case in cases:
        p = SubmapAlignParams(method=method, semantics_dim=D, submap_radius=15.0, **kw)
        reg, pools = _build(method, descriptor, dev, ctx)
        got = sa.submap_align_pools(p, [pools[0], pools[0]] if self_case else pools, io, registration=reg, num_solutions=2)
        want = stand_in(method, descriptor, p, self_case)
        _same(got, want, POSE); _same_hyps(got, want, POSE)
        print(name, "pairs", len(got.hypotheses), "edges", len(got.lc_edges["pairs"]))
        assert len(got.hypotheses) > 0

    # a session of three robots == submap_align_pools(num_solutions=2) per block
    p = SubmapAlignParams(method="gravity", semantics_dim=D, submap_radius=15.0, single_robot_lc_time_thresh=40.0)
    reg, pools = _build("gravity", None, dev, ctx)
    three = [pools[0], pools[1], pools[0]]
    blocks = [(0, 0), (0, 1), (1, 2)]
    got = sa.submap_align_session(p, three, blocks, io, registration=reg, num_solutions=2)
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        want = sa.submap_align_pools(q, [three[r], three[s]], io, registration=reg, num_solutions=2)
        _same(got[(r, s)], want, 1e-12); _same_hyps(got[(r, s)], want, 1e-12)

    # consistency with the existing path: no single scores, K = 1
    base = sa.submap_align_pools(p, pools, io, registration=reg)
    one = sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=1)
    n = base.clipper_num_associations
    assert len(base.lc_edges["pairs"]) >= 1 and (n[~np.isnan(n)] < 4).any(), "needs an accepted pair and one that is not"
    _same(one, base, 1e-12)
    # the device-prefilter plugin (clipper+prune): the prefilter's survivors ARE the list the plain solve is handed, so K = 1 is the
    # single-solution path here too — over the world of tests/test_gpu_prune_pools.py, whose planted 8 degree roll the tail's
    # tilt_thresh rejects on either path; and K = 2 keeps hypothesis 0
    import test_gpu_prune_pools as tp
    pp, pio, preg, _, ppools, _ = tp.build(ctx, dev)
    base = sa.submap_align_pools(pp, ppools, pio, registration=preg)
    one = sa.submap_align_pools(pp, ppools, pio, registration=preg, num_solutions=1)
    two = sa.submap_align_pools(pp, ppools, pio, registration=preg, num_solutions=2)
    assert len(base.lc_edges["pairs"]) >= 1
    _same(one, base, 1e-12)
    tilt = [key for key, h in one.hypotheses.items() if h[0][4] & 4]
    assert tilt, "the planted roll must fail the tilt check of hypothesis 0"
    for key, h in one.hypotheses.items():
        assert np.array_equal(h[0][0], two.hypotheses[key][0][0]) and h[0][3:5] == two.hypotheses[key][0][3:5]
    print("MNO_POOLS_OK")
    ctx.close()


@pytest.mark.gpu
def test_num_solutions_over_pools_and_session_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_pools_mno as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "MNO_POOLS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
