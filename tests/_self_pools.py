"""One robot closing loops against its own map over device-resident pools — TEST INFRASTRUCTURE shared by
tests/test_self_pools_cpu.py (stand-in contexts) and tests/test_gpu_self_pools.py (the device).

`two_lap_map()` drives the loop of synth.make_map twice: every segment of lap 1 is seen again on lap 2 as a NEW segment (its own
id, the centre a few cm off, the descriptor slightly off, first_seen / last_seen one lap later).  The time window of
[REF roman/map/map.py:315-320] keeps the laps apart inside a submap, so submaps of the same lap share segments with their
neighbours (and all of them with themselves), submaps of different laps share none but hold true matches.

`run_case()` runs submap_align_pools(p, [pool, pool]) and submap_align_grid on to_submaps() of the same pool (twice: two
independent sides); `compare()` holds the tolerances of tests/test_gpu_submap_align_pools.py and the conditions that keep the
comparison from passing vacuously."""
import copy

import numpy as np

import _shared_ids as si
from _stub_context import _view

D = 16
N_POSES, DT = 120, 2.0
LAP = N_POSES * DT                  # seconds per lap
TIME_THRESH = 230.0                 # single_robot_lc_time_thresh: shorter than a lap (240 s), longer than the time between the first and the last centre of a lap (224 s)
LC_THRESH = 4
CASES = [dict(name="roman-mean-semantic", method="roman", descriptor='mean_semantic', thresh=0.65),
         dict(name="gravity-no-descriptor", method="gravity", descriptor=None, thresh=0.0)]


def two_lap_map(seed=61, n_lap=300):
    """-> (segments, trajectory, times): lap 1 as synth.make_map places it, lap 2 behind it."""
    from roman_amd import synth
    segs, traj, times = synth.make_map(n_lap, D, seed=seed, n_poses=N_POSES, loop_radius=19.0, laps=1.0, dt=DT)
    rng = np.random.default_rng(seed + 1)
    again = []
    for k, s in enumerate(segs):
        q = copy.deepcopy(s)
        q.id = 5000 + k
        q.centroid = np.asarray(s.centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(s.centroid))
        v = np.asarray(s.semantic_descriptor, dtype=np.float64) + 0.02 * rng.standard_normal(D) / np.sqrt(D)
        q.semantic_descriptor = v / np.linalg.norm(v)
        q.first_seen, q.last_seen = s.first_seen + LAP, s.last_seen + LAP
        again.append(q)
    return segs + again, list(traj) + [np.array(T) for T in traj], np.concatenate([times, times + LAP])


def params_of(case):
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    p = SubmapAlignParams(method=case["method"], semantics_dim=D, submap_radius=15.0, submap_center_dist=15.0, submap_max_size=40,
                          submap_descriptor=case["descriptor"], submap_descriptor_thresh=case["thresh"],
                          single_robot_lc=True, single_robot_lc_time_thresh=TIME_THRESH)
    return p, sa.SubmapAlignIO(lc_association_thresh=LC_THRESH)


def build_pool(case, reg, ctx, device):
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p, _ = params_of(case)
    params = SubmapParams.from_submap_align_params(p)
    segs, traj, times = two_lap_map()
    pool = build_submap_pool(reg, MapTable.from_segments(reg, segs), submap_centers(traj, times, params), params, ctx=ctx, device=device)
    return pool, segs


def run_case(case, ctx, device, build_ctx=None, compute=None):
    """-> (result of the pools path, result of the grid path, the pool)."""
    from roman_amd.align import submap_align as sa
    p, io = params_of(case)
    reg = p.get_object_registration(); reg.set_context(ctx)
    pool, segs = build_pool(case, reg, build_ctx or ctx, device)
    got = sa.submap_align_pools(p, [pool, pool], io, registration=reg)
    want = sa.submap_align_grid(p, [pool.to_submaps(segs), pool.to_submaps(segs)], io, registration=reg, compute=compute)
    return got, want, pool


def shared_counts(pool):
    """(S, S) ids both submaps hold, (S,) sizes — over the non-empty submaps."""
    k = pool.nonempty
    sets = [set(pool.ids[s, :pool.count[s]].tolist()) for s in k]
    return np.array([[len(a & b) for b in sets] for a in sets]), np.array([len(a) for a in sets])


def conditions(case, want, pool):
    """What the grid path alone must show for the comparison to mean something."""
    n = want.clipper_num_associations
    S = n.shape[0]
    assert n.shape == (S, S) and 8 <= S <= 16, n.shape
    done = np.ones((S, S), dtype=bool)                   # registered: no skip distance, so every pair the descriptor gate lets through
    if case["descriptor"] is not None:
        sim = want.similarity_mat
        assert np.nanmin(np.abs(sim - case["thresh"])) > 1e-3, "a similarity sits on the threshold: choose another"
        done &= sim >= case["thresh"]
        assert (sim < case["thresh"]).any(), "the descriptor gate stops no pair"
    assert np.all(np.diag(n) == 0), "a submap against itself keeps segments"
    shared, size = shared_counts(pool)
    off = ~np.eye(S, dtype=bool)
    some = off & done & (shared > 0) & (shared < size[:, None]) & (shared < size[None, :])
    none = done & (shared == 0)
    assert some.sum() >= 3, "fewer than 3 registered off-diagonal pairs lost some but not all segments"
    assert none.sum() >= 3, "fewer than 3 registered pairs lost nothing"
    times = pool.centers.time[pool.nonempty]
    dt = np.abs(times[:, None] - times[None, :])
    lap = (times >= LAP).astype(int)
    acc = np.asarray(want.lc_edges["pairs"]).reshape(-1, 2)
    assert len(acc) >= 3 and np.all(lap[acc[:, 0]] != lap[acc[:, 1]]), "fewer than 3 accepted loop closures, or one inside a lap"
    assert ((n >= LC_THRESH) & (dt < TIME_THRESH)).any(), "the time gate stopped no pair with enough associations"
    assert np.all(dt[acc[:, 0], acc[:, 1]] >= TIME_THRESH)
    return dict(S=S, some=int(some.sum()), none=int(none.sum()), accepted=len(acc), gated=int(((n >= LC_THRESH) & (dt < TIME_THRESH)).sum()))


def compare(got, want):
    n = want.clipper_num_associations
    n0, n1 = n.shape
    assert np.array_equal(got.clipper_num_associations, n, equal_nan=True)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    for name in ("T_ij_mat", "T_ij_hat_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
    for name in ("clipper_angle_mat", "clipper_dist_mat", "submap_yaw_diff_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    assert (got.similarity_mat is None) == (want.similarity_mat is None)
    if want.similarity_mat is not None:
        np.testing.assert_allclose(got.similarity_mat, want.similarity_mat, rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
    np.testing.assert_allclose(got.lc_edges["t"], want.lc_edges["t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.lc_edges["q"], want.lc_edges["q"], rtol=0, atol=1e-12)


def shared_reduce_model(B, F, feats_ptr, region_row0, ids_ptr, off1, n1, off2, n2, keep_ptr, kept_ptr):
    """roman_shared_reduce_dev through raw addresses of host memory: tests/_shared_ids.mark for the lists, then the fixed slots."""
    total = int(np.sum(n1, dtype=np.int64) + np.sum(n2, dtype=np.int64))
    ids = _view(ids_ptr, (int(region_row0),), np.int64)
    feats = _view(feats_ptr, (int(region_row0) + total, F), np.float64)
    keep, kept = si.mark(ids, off1, n1, off2, n2)
    out_keep, out_kept = _view(keep_ptr, (total,), np.int32), _view(kept_ptr, (B, 2), np.int32)
    out_kept[:] = kept
    kb = 0
    for b, (k1, k2) in enumerate(si.kept_lists(keep, kept, n1, n2)):
        out_keep[kb:kb + len(k1)] = k1; out_keep[kb + n1[b]:kb + n1[b] + len(k2)] = k2
        if len(k1) != n1[b] or len(k2) != n2[b]:
            feats[region_row0 + kb:region_row0 + kb + len(k1)] = feats[off1[b] + k1]
            feats[region_row0 + kb + n1[b]:region_row0 + kb + n1[b] + len(k2)] = feats[off2[b] + k2]
        kb += int(n1[b]) + int(n2[b])
