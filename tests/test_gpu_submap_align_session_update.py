"""submap_align_session_update on the device: three small maps, a full first call on the pools cut back by two
submaps per robot, then two appending steps — after every call EQUAL to submap_align_session over the same pools: every matrix, the
associations, the edges and the hypotheses, bit for bit (a problem's result does not depend on the batch it runs in, and the list
gate writes the bits of the whole-grid gate).  torch holds the device memory, so the comparison runs in a process of its own with
torch imported first (as tests/test_gpu_submap_align_session.py does)."""
import subprocess
import sys

import pytest

D = 16
CASES = ["mean-semantic", "one-storage", "stacked", "aabb", "ransac", "two-solutions"]


def pools_of(name, reg, ctx, device):
    """-> (params, pools, registration, num_solutions): the pools of the whole-session tests, per case."""
    import test_gpu_submap_align_session as t0
    import test_gpu_submap_align_session_aabb as ta
    import test_gpu_submap_align_session_stacked as ts
    from roman_amd.align import RansacReg, SubmapAlignParams
    if name in ("mean-semantic", "two-solutions"):           # separately built pools, self blocks through roman_shared_reduce_dev
        p, pools = t0.make_pools(t0.CASES[0], reg, ctx, device)
        return p, pools, reg, 2 if name == "two-solutions" else None
    if name == "one-storage":                                # the pools of ONE build_session_pools call: row ranges of one tensor
        import _session as ss
        from roman_amd import synth
        from roman_amd.align.submaps import MapTable, SubmapParams, build_session_pools, submap_centers
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40,
                              submap_descriptor='mean_semantic', submap_descriptor_thresh=0.65, single_robot_lc_time_thresh=60.0)
        params = SubmapParams.from_submap_align_params(p)
        base = synth.make_map(300, D, seed=41, n_poses=60, dt=4.0)
        tables, centers = [], []
        for r, v in enumerate(t0.VIEWS):
            segs, traj, times = ss.robot_view(*base, r, d=D, keep=v["keep"], first_pose=v["first_pose"], last_pose=v["last_pose"])
            tables.append(MapTable.from_segments(reg, segs)); centers.append(submap_centers(traj, times, params))
        return p, build_session_pools(reg, tables, centers, params, ctx=ctx, device=device), reg, None
    if name == "stacked":
        p, pools = ts.make_pools(reg, ctx, device)
        return p, pools, reg, None
    ransac = name == "ransac"                                # "aabb": force-fill pools under the bounding-box gate; "ransac": the same pools, radius gate
    pools = ta.fill_pools(reg, ctx, device)
    p = SubmapAlignParams(method="ransac" if ransac else "roman", semantics_dim=D, force_fill_submaps=not ransac, submap_radius=ta.RADIUS, submap_max_size=24,
                          submap_overlap=8, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.65, single_robot_lc_time_thresh=60.0)
    if ransac:
        reg = RansacReg(max_iteration=2048, round=256); reg.set_context(ctx)
    return p, pools, reg, None


def run_case(name, ctx, device):
    import _session_update as su
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    roman = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); roman.set_context(ctx)
    p, final, reg, K = pools_of(name, roman, ctx, device)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=40.0)
    n = [len(q.count) for q in final]
    assert min(n) >= 4, n
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    state = sa.SessionAlignState()
    listed, registered, accepted = [], 0, 0
    for step in range(3):
        pools = final if step == 2 else [su.pool_prefix(q, m - 2 + step) for q, m in zip(final, n)]
        got = sa.submap_align_session_update(state, p, pools, None, None, io, registration=reg, num_solutions=K)
        want = sa.submap_align_session(p, pools, None, io, registration=reg, num_solutions=K)
        assert list(got) == list(want) == blocks
        for key in blocks:
            su.equal(got[key], want[key])
        listed.append((state.listed, state.total))
        registered = sum(len(w.timing_list) for w in want.values()); accepted = sum(len(w.lc_edges["pairs"]) for w in want.values())
        fresh = sum(len(g.timing_list) for g in got.values())
        assert fresh <= registered and (step == 0) == (state.listed == state.total), (step, listed)
    assert registered >= 6 and accepted >= 1, "hardly a pair aligned: the comparison would show nothing"
    if K is not None:
        assert sum(len(w.hypotheses) for w in want.values()) == registered
    print(f"{name}: listed / all pairs per step {listed}, {registered} pairs registered at the end, {accepted} accepted, submaps {n}")


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for name in CASES:
        run_case(name, ctx, dev)
    ctx.close()
    print("SESSION_UPDATE_OK")


@pytest.mark.gpu
def test_update_equals_the_full_session_call_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_session_update as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_UPDATE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
