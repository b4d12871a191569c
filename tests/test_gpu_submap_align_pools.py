"""submap_align_pools on the device: two small maps -> build_submap_pool x 2 -> submap_align_pools, against
submap_align_grid on to_submaps() of the SAME pools.  torch holds the device memory, so the comparison runs in a process of its
own with torch imported first (as tests/test_gpu_submaps.py::test_device_pools_feed_the_batch_calls does).

Exact: clipper_num_associations, robots_nearby_mat, every association array, the accepted pairs.  Poses and edges: 1e-12.  Angle
and distance matrices: 1e-9 (the tolerances of tests/test_gpu_ransac.py::test_through_the_plugin)."""
import subprocess
import sys

import numpy as np
import pytest

D = 16
# The descriptor threshold sits in a gap of the similarities of these maps (the nearest lies more than 1e-3 away: the two paths
# add the 16 products in different orders), the skip distance in a gap of the centre distances.
CASES = [dict(name="roman-descriptor-skip", method="roman", descriptor='mean_semantic', thresh=0.65, skip=40.0, first_empty=False),
         dict(name="gravity-first-centre-empty", method="gravity", descriptor=None, thresh=0.0, skip=np.inf, first_empty=True),
         dict(name="roman-descriptor-first-centre-empty", method="roman", descriptor='mean_semantic', thresh=0.65, skip=np.inf, first_empty=True)]


def make_maps(first_empty):
    """The same place mapped twice (cross pairs have true matches): about 300 segments, 7 centres 30 m apart; `first_empty`
    opens the trajectory 400 m away, where no segment is."""
    from roman_amd import synth
    maps = []
    for seed in (41, 41):
        segs, traj, times = synth.make_map(300, D, seed=seed, n_poses=60, dt=4.0)
        if first_empty:
            far = np.array(traj[0]); far[:3, 3] += (400.0, 0.0, 0.0)
            traj = [far] + list(traj); times = np.concatenate([[times[0] - 4.0], times])
        maps.append((segs, traj, times))
    return maps


def run_case(case, ctx, device, build_ctx=None, compute=None):
    """-> (result of the pools path, result of the grid path, the pools)."""
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p = SubmapAlignParams(method=case["method"], semantics_dim=D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40,
                          submap_descriptor=case["descriptor"], submap_descriptor_thresh=case["thresh"])
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=case["skip"])
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    pools, segs = [], []
    for sg, traj, times in make_maps(case["first_empty"]):
        table = MapTable.from_segments(reg, sg)
        pools.append(build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=build_ctx or ctx, device=device))
        segs.append(sg)
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pools, segs)], io, registration=reg, compute=compute)
    return got, want, pools


def compare(case, got, want, pools):
    n = want.clipper_num_associations
    n0, n1 = n.shape
    assert 5 <= n0 <= 8 and 5 <= n1 <= 8, (n0, n1)
    if case["first_empty"]:
        assert pools[0].count[0] == 0 and pools[0].nonempty[0] == 1, "the first centre is not empty"
    skipped = np.isnan(want.T_ij_hat_mat[:, :, 0, 0]) & (n == 0) & np.isnan(want.similarity_mat if want.similarity_mat is not None else np.full(n.shape, 0.0))
    if case["descriptor"] is not None:
        sim = want.similarity_mat
        assert np.nanmin(np.abs(sim - case["thresh"])) > 1e-3, "a similarity sits on the threshold: choose another"
        gated = sim < case["thresh"]
        todo = sim >= case["thresh"]
        assert gated.any() and todo.any(), "the threshold does not split the pairs"
        if np.isfinite(case["skip"]):
            assert np.isnan(sim).any() and skipped.any(), "no pair was skipped for distance: the three classes do not all occur"
    assert np.array_equal(got.clipper_num_associations, n, equal_nan=True)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert (n >= 4).sum() >= 3, "hardly a pair of the grid aligned: the comparison would show nothing"
    for name in ("T_ij_mat", "T_ij_hat_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
    for name in ("clipper_angle_mat", "clipper_dist_mat", "submap_yaw_diff_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    assert (got.similarity_mat is None) == (want.similarity_mat is None)
    if want.similarity_mat is not None:
        np.testing.assert_allclose(got.similarity_mat, want.similarity_mat, rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"]) and len(want.lc_edges["pairs"]) >= 3
    np.testing.assert_allclose(got.lc_edges["t"], want.lc_edges["t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.lc_edges["q"], want.lc_edges["q"], rtol=0, atol=1e-12)


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for case in CASES:
        got, want, pools = run_case(case, ctx, dev)
        compare(case, got, want, pools)
        print(f"{case['name']}: {want.clipper_num_associations.shape} grid, {len(got.timing_list)} pairs registered, {len(want.lc_edges['pairs'])} loop closures")
    ctx.close()
    print("POOLS_GRID_OK")


@pytest.mark.gpu
def test_pools_path_equals_grid_path_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_pools as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "POOLS_GRID_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
