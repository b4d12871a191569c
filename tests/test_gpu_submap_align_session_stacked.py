"""submap_align_session with 'stacked_frame_descriptors' on the device: three small maps ->
build_submap_pool(frames=...) x 3 -> ONE session call, against submap_align_pools called per robot pair on the SAME pools (self blocks
through roman_shared_reduce_dev on both sides).  torch holds the device memory, so the comparison runs in a process of its own with
torch imported first (as tests/test_gpu_submap_align_session.py does).

The records, the edges and the matrices as tests/_session.compare holds them between two results of one block; similarity_mat bit
for bit: roman_session_stacked_sim_dev promises roman_stacked_sim_dev's bits.  The reference side must hold a block with a GATED and a
TODO pair, and no similarity within 1e-3 of the threshold."""
import subprocess
import sys

import numpy as np
import pytest

D, DF = 16, 24
MODE = 'stacked_frame_descriptors'
THRESH = 0.8            # the reference demo's submap_descriptor_thresh; frame_descriptor_dist 10.0 likewise
VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None, max_size=40), dict(keep=0.85, first_pose=8, last_pose=None, max_size=36),
         dict(keep=0.9, first_pose=0, last_pose=50, max_size=44)]


def make_pools(reg, ctx, device):
    """The three views of tests/test_gpu_submap_align_session.py with frame descriptors: one vector per pose of the drive,
    independent from pose to pose (submaps that share no frame are dissimilar), every robot's copy with noise of its own; the
    robots see other stretches of the drive, so their frame tables differ in length."""
    import dataclasses
    import _session as ss
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align.submaps import FrameTable, MapTable, SubmapParams, build_submap_pool, submap_centers
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40, submap_descriptor=MODE,
                          frame_descriptor_dist=10.0, submap_descriptor_thresh=THRESH, single_robot_lc_time_thresh=60.0)
    base = synth.make_map(300, D, seed=41, n_poses=60, dt=4.0)
    per_pose = np.random.default_rng(43).normal(0.0, 1.0, (60, DF))
    pools = []
    for r, v in enumerate(VIEWS):
        params = dataclasses.replace(SubmapParams.from_submap_align_params(p), max_size=v["max_size"])
        segs, traj, times = ss.robot_view(*base, r, keep=v["keep"], first_pose=v["first_pose"], last_pose=v["last_pose"], d=D)
        desc = per_pose[slice(v["first_pose"], v["last_pose"])] + 0.1 * np.random.default_rng(44 + r).normal(0.0, 1.0, (len(traj), DF))
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, segs), submap_centers(traj, times, params), params, ctx=ctx, device=device,
                                       frames=FrameTable.from_map(traj, times, list(desc))))
    assert len({int(q.pool.shape[0]) for q in pools}) == 3 and len({int(q.cap) for q in pools}) == 3, "two robots have pools of one shape"
    assert len({int(q.frame_desc_dev.shape[0]) for q in pools}) == 3, "two robots have frame tables of one length"
    return p, pools


def run_case(ctx, device, build_ctx=None, exact_sim=True):
    import copy
    import _session as ss
    from roman_amd.align import submap_align as sa
    from roman_amd.align import SubmapAlignParams
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); reg.set_context(ctx)
    p, pools = make_pools(reg, build_ctx or ctx, device)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=40.0)
    got = sa.submap_align_session(p, pools, None, io, registration=reg)
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    assert list(got) == blocks
    aligned = edges = both = 0
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        want = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
        ss.compare(got[(r, s)], want)
        n, sim = want.clipper_num_associations, want.similarity_mat
        assert np.array_equal(np.isnan(got[(r, s)].T_ij_hat_mat[:, :, 0, 0]), np.isnan(want.T_ij_hat_mat[:, :, 0, 0]))
        if exact_sim:
            assert np.array_equal(got[(r, s)].similarity_mat, sim, equal_nan=True), (r, s)
        with np.errstate(invalid="ignore"):
            assert np.nanmin(np.abs(sim - THRESH)) > 1e-3, "a similarity sits on the threshold: choose another"
            both += int((sim < THRESH).any() and (sim >= THRESH).any())
        aligned += int((n >= 4).sum()); edges += len(want.lc_edges["pairs"])
        if r == s:
            assert np.all(np.diag(n) == 0), "a submap against itself keeps segments: the shared-segment removal did not run"
    assert both >= 1, "no block of the reference holds a GATED and a TODO pair: the similarity decides nothing"
    assert aligned >= 6 and edges >= 3, "hardly a pair aligned: the comparison would show nothing"
    print(f"stacked session: {aligned} pairs aligned, {edges} loop closures, {both} of {len(blocks)} blocks hold a GATED and a TODO pair, "
          f"frames per robot {[int(q.frame_desc_dev.shape[0]) for q in pools]}")


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    run_case(ctx, dev)
    ctx.close()
    print("SESSION_STACKED_OK")


@pytest.mark.gpu
def test_session_equals_pools_per_block_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_session_stacked as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_STACKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
