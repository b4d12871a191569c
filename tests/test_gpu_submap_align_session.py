"""submap_align_session on the device: three small maps -> build_submap_pool x 3 -> ONE session call, against
submap_align_pools called per robot pair on the SAME pools.  torch holds the device memory, so the comparison runs in a process of
its own with torch imported first (as tests/test_gpu_submap_align_pools.py does).

Exact: the nearby matrix, the TODO sets (the pairs with a count), the association counts and arrays, the accepted pairs.  Poses and
edges: 1e-12; angle and distance matrices: 1e-9 — the bounds tests/test_gpu_submap_align_pools.py holds between the pools path and the
grid path (tests/_session.compare)."""
import subprocess
import sys

import numpy as np
import pytest

D = 16
CASES = [dict(name="roman-mean-semantic", method="roman", descriptor='mean_semantic', thresh=0.65, skip=40.0, far=None),
         dict(name="gravity-no-descriptor-one-robot-far", method="gravity", descriptor=None, thresh=0.0, skip=60.0, far=2)]


VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None, max_size=40), dict(keep=0.85, first_pose=8, last_pose=None, max_size=36),
         dict(keep=0.9, first_pose=0, last_pose=50, max_size=44)]


def make_pools(case, reg, ctx, device):
    """The same place mapped three times (about 300 segments, centres 30 m apart), every robot with its OWN view of it
    (tests/_session.robot_view: other segments, centres a few cm off, another stretch of the drive, ids of its own) and its own
    pool shape (other cap): no two pools hold the same rows, the same number of rows or of submaps, so a problem that read
    another robot's rows would show.  Robot `far` maps the place 500 m away: no pair of its blocks with another robot lies
    within the skip distance."""
    import dataclasses
    import _session as ss
    from roman_amd import synth
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    from roman_amd.align import SubmapAlignParams
    p = SubmapAlignParams(method=case["method"], semantics_dim=D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40,
                          submap_descriptor=case["descriptor"], submap_descriptor_thresh=case["thresh"], single_robot_lc_time_thresh=60.0)
    base = synth.make_map(300, D, seed=41, n_poses=60, dt=4.0)
    pools = []
    for r, v in enumerate(VIEWS):
        params = dataclasses.replace(SubmapParams.from_submap_align_params(p), max_size=v["max_size"])
        segs, traj, times = ss.robot_view(*base, r, keep=v["keep"], first_pose=v["first_pose"], last_pose=v["last_pose"], d=D)
        if r == case["far"]:
            for q in segs:
                q.centroid = np.asarray(q.centroid, dtype=np.float64) + np.array([500.0, 0.0, 0.0])[:np.size(q.centroid)].reshape(np.shape(q.centroid))
            for T in traj:
                T[:3, 3] += (500.0, 0.0, 0.0)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, segs), submap_centers(traj, times, params), params, ctx=ctx, device=device))
    assert len({int(q.pool.shape[0]) for q in pools}) == 3 and len({int(q.cap) for q in pools}) == 3, "two robots have pools of one shape"
    return p, pools


def run_case(case, ctx, device):
    import copy
    import _session as ss
    from roman_amd.align import submap_align as sa
    from roman_amd.align import SubmapAlignParams
    reg = SubmapAlignParams(method=case["method"], semantics_dim=D).get_object_registration(); reg.set_context(ctx)
    p, pools = make_pools(case, reg, ctx, device)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=case["skip"])
    got = sa.submap_align_session(p, pools, None, io, registration=reg)
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    assert list(got) == blocks
    aligned = edges = 0
    empty_blocks = []
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        want = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
        ss.compare(got[(r, s)], want)
        n = want.clipper_num_associations
        assert 4 <= n.shape[0] <= 8 and 4 <= n.shape[1] <= 8, n.shape
        assert np.array_equal(np.isnan(got[(r, s)].T_ij_hat_mat[:, :, 0, 0]), np.isnan(want.T_ij_hat_mat[:, :, 0, 0]))
        aligned += int((n >= 4).sum()); edges += len(want.lc_edges["pairs"])
        if len(want.timing_list) == 0:
            empty_blocks.append((r, s))
        if r == s:
            assert np.all(np.diag(n) == 0), "a submap against itself keeps segments: the shared-segment removal did not run"
        if case["descriptor"] is not None:
            sim = want.similarity_mat
            assert np.nanmin(np.abs(sim - case["thresh"])) > 1e-3, "a similarity sits on the threshold: choose another"
    assert aligned >= 6 and edges >= 3, "hardly a pair aligned: the comparison would show nothing"
    if case["far"] is not None:
        assert empty_blocks == [(0, 2), (1, 2)], empty_blocks
    print(f"{case['name']}: {aligned} pairs aligned, {edges} loop closures, blocks without a pair: {empty_blocks}")


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for case in CASES:
        run_case(case, ctx, dev)
    ctx.close()
    print("SESSION_OK")


@pytest.mark.gpu
def test_session_equals_pools_per_block_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_session as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
