"""submap_align_session in AABB mode and with a RansacReg on the device: three maps -> three pools -> ONE session
call, against submap_align_pools called per robot pair on the SAME pools — EXACTLY (tests/_session_aabb.exact: every matrix, every
association list, the similarity and the edges bit for bit).  torch holds the device memory, so the comparison runs in a process
of its own with torch imported first (as tests/test_gpu_submap_align_session.py does).

  fill-mean-semantic   force-fill pools differing in rows, submaps and cap, 'mean_semantic', every r <= s (self blocks included)
  fill-stacked         the same maps cut into force-fill pools WITH frame tables (build_submap_pool(fill=..., frames=...)),
                       'stacked_frame_descriptors': roman_session_stacked_sim_dev in front of the bounding-box gate
  stacked-no-radius    the frame-descriptor pools of tests/test_gpu_submap_align_session_stacked.py with submap_radius None
  ransac-radius/-aabb  the force-fill pools with a RansacReg, the radius gate and the bounding-box gate

Asserted on the reference side before comparing, so that the test cannot pass vacuously: two blocks keep a TODO pair; a pair's NEARBY
under boxes differs from dist < 2 * radius with the radius of the parameters (a gate instantiated without AABB would show) — in the
case without a radius such a gate would read -1 and call nothing NEARBY, so there a NEARBY pair and a pair that is not are asked
for —; a pair is accepted and one is rejected (RANSAC included)."""
import subprocess
import sys

import numpy as np
import pytest

D, DF = 16, 24
MODE = 'stacked_frame_descriptors'
RADIUS = 15.0
STACKED_THRESH = 0.8
STACKED_MAX_SIZE = (24, 18, 28)        # (after dropping the segments a stretch did not see: three different numbers of submaps)
VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None, max_size=24), dict(keep=0.85, first_pose=8, last_pose=None, max_size=20),
         dict(keep=0.9, first_pose=0, last_pose=50, max_size=28)]
CASES = ["fill-mean-semantic", "fill-stacked", "stacked-no-radius", "ransac-radius", "ransac-aabb"]


def fill_pools(reg, ctx, device, fill_ctx=None, stacked=False):
    """The same place mapped three times (120 segments), every robot with its own view of it (tests/_session.robot_view) cut into
    force-fill slices of its own length: no two pools hold the same rows, the same number of rows or of submaps, or the same cap.
    `stacked`: with frame tables — one descriptor per pose of the drive, independent from pose to pose (submaps that share no frame
    are dissimilar), every robot's copy with noise of its own; the robots see other stretches, so their frame tables differ in length."""
    import _session as ss
    from roman_amd import synth
    from roman_amd.align.submaps import FillSubmapParams, FrameTable, MapTable, build_submap_pool, fill_centers
    base = synth.make_map(120, D, seed=41, n_poses=60, dt=4.0)
    per_pose = np.random.default_rng(43).normal(0.0, 1.0, (60, DF))
    pools = []
    for r, v in enumerate(VIEWS):
        segs, traj, times = ss.robot_view(*base, r, keep=v["keep"], first_pose=v["first_pose"], last_pose=v["last_pose"], d=D)
        if stacked:                                          # a submap needs a frame in its time span: the segments this stretch of the drive saw
            tt = np.asarray(times, dtype=np.float64)
            segs = [q for q in segs if np.any((tt >= float(q.first_seen)) & (tt <= float(q.last_seen)))]
        table = MapTable.from_segments(reg, segs)
        fp = FillSubmapParams(STACKED_MAX_SIZE[r], 8, MODE, 10.0) if stacked else FillSubmapParams(v["max_size"], 8, 'mean_semantic')
        centers, slices = fill_centers(table, traj, times, fp)
        frames = None
        if stacked:
            desc = per_pose[slice(v["first_pose"], v["last_pose"])] + 0.1 * np.random.default_rng(44 + r).normal(0.0, 1.0, (len(traj), DF))
            frames = FrameTable.from_map(traj, times, list(desc))
        pools.append(build_submap_pool(reg, table, centers, fp, ctx=fill_ctx or ctx, device=device, fill=slices, frames=frames))
    assert len({int(q.pool.shape[0]) for q in pools}) == 3 and len({int(q.cap) for q in pools}) == 3 and len({len(q.nonempty) for q in pools}) == 3
    assert not stacked or len({int(q.frame_desc_dev.shape[0]) for q in pools}) == 3, "two robots have frame tables of one length"
    return pools


def centre_distances(pa, pb):
    a = np.array([pa.centers.pose_flu[s][:3, 3] for s in pa.nonempty]); b = np.array([pb.centers.pose_flu[s][:3, 3] for s in pb.nonempty])
    return np.linalg.norm(a[:, None, :] - b[None, :, :], axis=2)


def run_case(name, ctx, device, fill_ctx=None):
    import copy
    import _session_aabb as sx
    from roman_amd.align import RansacReg, SubmapAlignParams
    from roman_amd.align import submap_align as sa
    roman = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); roman.set_context(ctx)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=40.0)
    aabb = name != "ransac-radius"
    if name == "stacked-no-radius":
        import test_gpu_submap_align_session_stacked as st
        p, pools = st.make_pools(roman, fill_ctx or ctx, device)
        p.submap_radius = None
        reg = roman
    else:
        stacked = name == "fill-stacked"
        pools = fill_pools(roman, ctx, device, fill_ctx, stacked)
        ransac = name.startswith("ransac")
        p = SubmapAlignParams(method="ransac" if ransac else "roman", semantics_dim=D, force_fill_submaps=aabb, submap_radius=RADIUS, submap_max_size=24,
                              submap_overlap=8, submap_descriptor=MODE if stacked else 'mean_semantic', frame_descriptor_dist=10.0 if stacked else None,
                              submap_descriptor_thresh=STACKED_THRESH if stacked else 0.65, single_robot_lc_time_thresh=60.0)
        reg = roman
        if ransac:
            reg = RansacReg(max_iteration=2048, round=256); reg.set_context(ctx)
    got = sa.submap_align_session(p, pools, None, io, registration=reg)
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    assert list(got) == blocks
    want = {}
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        want[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
    # ---- the conditions, on the reference side ----
    with_todo = sum(len(w.timing_list) > 0 for w in want.values())
    registered = sum(len(w.timing_list) for w in want.values())
    accepted = sum(len(w.lc_edges["pairs"]) for w in want.values())
    assert with_todo >= 2, "fewer than two blocks keep a TODO pair"
    if aabb:
        differs = sum(int(((~np.isnan(w.robots_nearby_mat)) != (centre_distances(pools[r], pools[s]) < 2 * RADIUS)).sum()) for (r, s), w in want.items())
        if p.submap_radius is not None:
            assert differs >= 1, "NEARBY under boxes equals dist < 2 * radius for every pair: a gate without AABB would pass"
        else:
            # no radius in the parameters: a gate without AABB would read radius -1 and call nothing NEARBY; these pools' boxes (radius
            # 15 m around centres 30 m apart) agree with dist < 30 m, so the pairs that differ are those of the force-fill cases
            near = np.concatenate([~np.isnan(w.robots_nearby_mat).reshape(-1) for w in want.values()])
            assert near.any() and (~near).any(), "every pair or no pair is NEARBY: the gate would show nothing"
    else:
        differs = 0
    assert accepted >= 1 and accepted < registered, "no pair is accepted, or none is rejected"
    if name == "fill-stacked":                               # the similarity decides something: a block with a GATED and a TODO pair, none on the threshold
        with np.errstate(invalid="ignore"):
            assert any((w.similarity_mat < STACKED_THRESH).any() and (w.similarity_mat >= STACKED_THRESH).any() for w in want.values())
            assert min(np.nanmin(np.abs(w.similarity_mat[np.isfinite(w.similarity_mat)] - STACKED_THRESH)) for w in want.values()) > 1e-3
    for key in blocks:
        sx.exact(got[key], want[key])
        assert got[key].submap_align_params.single_robot_lc == (key[0] == key[1])
    print(f"{name}: {with_todo} blocks with a TODO pair, {registered} pairs registered, {accepted} accepted, {differs} pairs whose NEARBY differs from the radius gate, "
          f"submaps {[len(q.nonempty) for q in pools]}, caps {[int(q.cap) for q in pools]}")


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for name in CASES:
        run_case(name, ctx, dev)
    ctx.close()
    print("SESSION_AABB_OK")


@pytest.mark.gpu
def test_session_equals_pools_per_block_in_aabb_mode_and_with_ransac_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_session_aabb as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_AABB_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
