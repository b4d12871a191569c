"""Force-fill submaps, the boxes of a pool and the bounding-box gate on the device against the NumPy restatement
of the contract (tests/_fill_boxes_oracle.py), through the C ABI, and submap_align_pools in AABB mode against submap_align_grid on
to_submaps() of the same pools.

Exact: boxes (min and max of the same four rounded operations per component), pool rows, count, src, ids and mean_semantic of the
gather, flags, pairs (content and order), n_todo, enable.  dist, sim, yaw_deg, T_ij, T_ref: the tolerances of
tests/test_gpu_grid_gate.py (1e-12 * max(1, |x|)).  End to end: the tolerances of tests/test_gpu_submap_align_pools.py."""
import subprocess
import sys

import numpy as np
import pytest

import _fill_boxes_oracle as fo
import _frame_desc_oracle as fdo
import _grid_gate_oracle as go
import test_gpu_grid_gate as tg
from roman_amd import _abi
from roman_amd.runtime import frame_select_params, grid_gate_params, submap_desc_dtype

D = 16


def general_pose(rng):
    from scipy.spatial.transform import Rotation as Rot
    T = np.eye(4)
    T[:3, :3] = Rot.from_euler('ZYX', [rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)]).as_matrix()
    T[:3, 3] = rng.uniform(-30, 30, 3)
    return T


# ---------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pose", ["yaw", "general"])
def test_boxes_bit_for_bit(ctx, pose):
    """cap 70: a wave takes a submap's rows in two steps; counts around the wave width; an empty submap is (+inf x 3, -inf x 3)."""
    rng = np.random.default_rng(11 if pose == "yaw" else 12)
    cap, F, count = 70, 5, np.array([0, 1, 63, 64, 65, 70], np.int32)
    S = len(count)
    pool = rng.uniform(-40.0, 40.0, (S * cap, F))                            # rows beyond a count hold values that would move the box
    T = np.array([go.yaw_pose(rng.uniform(-np.pi, np.pi), rng.uniform(-30, 30, 3)) if pose == "yaw" else general_pose(rng) for _ in range(S)])
    want = fo.boxes_oracle(pool, cap, count, T)
    got = ctx.submap_boxes(pool, cap, count, T)
    assert got.shape == (S, 6) and got.tobytes() == want.tobytes()
    assert np.all(np.isposinf(got[0, :3])) and np.all(np.isneginf(got[0, 3:]))
    assert np.all(got[1, :3] == got[1, 3:])                                  # one row: a point


# ---------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------
def planted_grid(S0, S1, d, seed):
    """Identity rotations and integer centres; side 1's boxes are planted against side 0's: touching exactly along x (NEARBY),
    separated by one ulp (clear), overlapping, or far away."""
    rng = np.random.default_rng(seed)
    a, b = go.random_side(rng, S0, max(d, 1)), go.random_side(rng, S1, max(d, 1))
    a["pos"] = np.stack([10.0 * np.arange(S0), np.zeros(S0), np.zeros(S0)], axis=1)
    box0 = np.hstack([a["pos"] - 2.0, a["pos"] + 2.0])
    box1 = np.zeros((S1, 6)); kinds = []
    for j in range(S1):
        i, kind = j % S0, ("touch", "ulp", "overlap", "far")[j % 4]
        lo = box0[i, :3].copy(); hi = box0[i, 3:].copy()
        if kind == "touch":
            lo[0] = box0[i, 3]; hi[0] = lo[0] + 3.0
        elif kind == "ulp":
            lo[0] = np.nextafter(box0[i, 3], np.inf); hi[0] = box0[i, 3] + 3.0
        elif kind == "overlap":
            lo[0] += 1.0; hi[0] += 1.0
        else:
            lo[1] += 1000.0; hi[1] += 1000.0
        box1[j] = np.concatenate([lo, hi]); kinds.append((i, kind))
    b["pos"] = np.round((box1[:, :3] + box1[:, 3:]) / 2.0)
    for side in (a, b):
        side["T_w"] = np.array([go.yaw_pose(0.0, p) for p in side["pos"]])
        if d == 0:
            side["desc"] = None
    return a, b, box0, box1, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["none", "vector", "sim_in"])
@pytest.mark.parametrize("S0,S1", [(5, 7), (65, 3)])
def test_gate_against_the_oracle(ctx, S0, S1, variant):
    d = 16 if variant == "vector" else 0
    a, b, box0, box1, kinds = planted_grid(S0, S1, d, 900 + S0)
    gate = dict(skip_distance=35.0 if S0 == 5 else np.inf, desc_thresh=0.6 if variant != "none" else 0.0, single_robot_lc=True, lc_time_thresh=60.0)
    sim_in = np.random.default_rng(5).uniform(0.2, 0.95, (S0, S1)) if variant == "sim_in" else None
    o = fo.aabb_gate_oracle(a, b, box0, box1, sim_in=sim_in, **gate)
    near = (o["flags"] & go.NEARBY) != 0
    for j, (i, kind) in enumerate(kinds):                                    # what was planted is what the oracle says
        assert near[i, j] == (kind in ("touch", "overlap")), (i, j, kind)
    assert 0 < near.sum() < near.size and 0 < o["n_todo"] and (variant == "none" or o["n_todo"] < S0 * S1)
    B = S0 * S1
    F = tg.FILL
    P = grid_gate_params(None, desc_dim=d, **gate)                           # (the radius is "none": -1 is not read)
    r = ctx.grid_gate_aabb(P, box0, box1, a["pos"], a["T_w"], b["pos"], b["T_w"], time0=a["time"], time1=b["time"], desc0=a["desc"], desc1=b["desc"],
                           sim_in=sim_in, pairs=np.full((B, 2), F["pairs"], np.int32), T_ref=np.full((B, 4, 4), F["T_ref"], np.float64),
                           enable=np.full(B, F["enable"], np.int32))
    got = dict(dist=r.dist, flags=r.flags, yaw_deg=r.yaw_deg, sim=r.sim, T_ij=r.T_ij, pairs=r.pairs, T_ref=r.T_ref, enable=r.enable,
               n_todo=np.array([r.n_todo]))
    tg.check(o, got, f"aabb {S0}x{S1} {variant}")
    assert np.array_equal(np.isnan(got["yaw_deg"]), ~near)                   # the yaw of NEARBY pairs only


@pytest.mark.gpu
def test_gate_entry_validation(ctx):
    """New entries validate as their neighbours do; the radius gate keeps answering ROMAN_E_UNSUPPORTED for "no radius"."""
    import ctypes as C
    lib = _abi.load_library()
    buf = np.zeros(4096, np.float64)
    v = C.c_void_p(buf.ctypes.data)
    h = ctx._h
    P = grid_gate_params(None)
    args = lambda box0=v, box1=v, sim_in=None, n_todo=v: ([v] * 10 + [v] * 8 + [n_todo, box0, box1, sim_in])
    assert lib.roman_grid_gate_aabb(h, C.byref(P), 2, 2, *args(box0=None)) == _abi.ROMAN_E_INVALID
    assert lib.roman_grid_gate_aabb(h, C.byref(P), -1, 2, *args()) == _abi.ROMAN_E_INVALID
    assert lib.roman_grid_gate_aabb(h, C.byref(P), 2, 2, *args(n_todo=None)) == _abi.ROMAN_E_INVALID
    assert lib.roman_grid_gate_aabb_dev(h, C.byref(P), 1 << 14, 1 << 14, *args()) == _abi.ROMAN_E_TOO_LARGE
    Pd = grid_gate_params(None, desc_dim=4)
    assert lib.roman_grid_gate_aabb(h, C.byref(Pd), 2, 2, *args(sim_in=v)) == _abi.ROMAN_E_INVALID       # a given similarity wants desc_dim 0
    Pr = grid_gate_params(None); Pr.reserved1 = 1
    assert lib.roman_grid_gate_aabb(h, C.byref(Pr), 2, 2, *args()) == _abi.ROMAN_E_INVALID
    assert lib.roman_grid_gate(h, C.byref(P), 2, 2, *([v] * 19)) == _abi.ROMAN_E_UNSUPPORTED
    assert lib.roman_submap_boxes(h, -1, 3, 4, v, v, v, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_submap_boxes(h, 2, 2, 4, v, v, v, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_submap_boxes(h, 2, 3, 0, v, v, v, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_submap_boxes_dev(h, 2, 3, 4, v, None, v, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_submap_boxes(h, 0, 3, 4, None, None, None, None) == _abi.ROMAN_OK
    cnt = np.array([5, 0], np.int32); src = np.zeros(8, np.int32)
    ci, si = C.c_void_p(cnt.ctypes.data), C.c_void_p(src.ctypes.data)
    fill = lambda *a: lib.roman_submaps_fill(h, *a)
    assert fill(3, 4, 10, 5, v, None, 2, v, ci, si, v, None, 0, None) == _abi.ROMAN_E_INVALID             # a count beyond its slot
    cnt[0] = 2; src[1] = 10
    assert fill(3, 4, 10, 5, v, None, 2, v, ci, si, v, None, 0, None) == _abi.ROMAN_E_INVALID             # a row that is no map index
    src[1] = 0
    assert fill(4, 4, 10, 5, v, None, 2, v, ci, si, v, None, 0, None) == _abi.ROMAN_E_INVALID             # point_dim
    assert fill(3, 4, 10, 5, v, None, 2, v, ci, si, v, v, 0, None) == _abi.ROMAN_E_INVALID                # ids_out without seg_ids
    assert fill(3, 4, 10, 5, v, None, 2, v, ci, si, v, None, 3, None) == _abi.ROMAN_E_INVALID             # desc_dim > F - 3
    assert lib.roman_submaps_fill_dev(h, 3, 4, 10, 5, v, None, 2, v, None, si, v, None, 0, None) == _abi.ROMAN_E_INVALID
    assert fill(3, 4, 10, 5, v, None, 0, None, None, None, None, None, 0, None) == _abi.ROMAN_OK


# ---------------------------------------------------------------------------------------------
# the gather of force-fill slices
# ---------------------------------------------------------------------------------------------
def tied_map(rng, N, F):
    """A map table whose reference times tie in places (exact copies of another segment's times)."""
    feats = rng.standard_normal((N, F)); feats[:, :3] = rng.uniform(-30, 30, (N, 3))
    t0 = rng.uniform(0.0, 200.0, N)
    times = np.stack([t0, t0 + rng.uniform(0.0, 10.0, N)], axis=1)
    for k in (3, 4, 11, 17):
        times[k] = times[k - 2]
    return np.ascontiguousarray(feats), times, np.arange(N, dtype=np.int64) * 7 + 1000


@pytest.mark.gpu
@pytest.mark.parametrize("max_size,overlap,point_dim", [(8, 3, 3), (8, 0, 3), (30, 5, 3), (8, 3, 2)])
def test_fill_gather_bit_for_bit(ctx, max_size, overlap, point_dim):
    rng = np.random.default_rng(100 + max_size + overlap)
    N, d = 23, 4
    F = 3 + 4 + d
    feats, times, ids = tied_map(rng, N, F)
    traj_times = np.arange(0.0, 220.0, 7.0)
    slices, mean, index = fo.fill_slices(times, traj_times, max_size, overlap)
    S = len(slices)
    assert S == {(8, 3): 5, (8, 0): 3, (30, 5): 1}[(max_size, overlap)] and len(slices[-1]) == {(8, 3): 3, (8, 0): 7, (30, 5): 23}[(max_size, overlap)]
    key = (times[:, 0] + times[:, 1]) / 2.0
    assert overlap or np.array_equal(np.sort(np.concatenate(slices)), np.arange(N))       # without overlap the slices partition the map
    assert any(key[a] == key[b] and a < b for s in slices for a, b in zip(s[:-1], s[1:])), "no tie inside a slice: the stable order is not exercised"
    descs = np.zeros(S, dtype=submap_desc_dtype())
    for s in range(S):
        descs[s]["T_center_odom"] = np.linalg.inv(general_pose(rng))
    want = fo.fill_oracle(feats, descs, slices, max_size, point_dim=point_dim, seg_ids=ids, desc_dim=d)
    r = ctx.submaps_fill(point_dim, max_size, feats, descs, want["count"], want["src"], seg_ids=ids, desc_dim=d)
    Fo = point_dim + F - 3
    assert r.pool.shape == (S * max_size, Fo)
    for s in range(S):
        n = int(want["count"][s])
        assert r.pool[s * max_size:s * max_size + n].tobytes() == want["rows"][s].tobytes(), s
        assert np.all(r.pool[s * max_size + n:(s + 1) * max_size] == 0.0)     # rows beyond the count are not written
        assert np.array_equal(r.ids[s * max_size:s * max_size + n], want["ids"][s]) and np.all(r.ids[s * max_size + n:(s + 1) * max_size] == -1)
    assert r.desc.tobytes() == want["desc"].tobytes()
    assert np.array_equal(r.count, want["count"]) and np.array_equal(r.src.reshape(S, max_size), want["src"])
    # roman_frame_select_dev reads the count and src of such a pool as it reads roman_submaps_dev's
    frame_times = np.arange(0.0, 215.0, 2.5); frame_desc = rng.standard_normal((len(frame_times), 6))
    fw = fdo.frame_select_oracle(want["count"], want["src"], times, frame_times, frame_desc=frame_desc, want_mean=True)
    fr = ctx.frame_select(frame_select_params(None, True), want["count"], want["src"], times, frame_times, frame_desc=frame_desc)
    assert np.array_equal(fr.mask, fw["mask"]) and np.array_equal(fr.n_sel, fw["n_sel"]) and fr.span.tobytes() == fw["span"].tobytes()
    assert fr.n_sel.min() > 0 and fr.mean.tobytes() == fw["mean"].tobytes()


# ---------------------------------------------------------------------------------------------
# end to end: submap_align_pools in AABB mode against submap_align_grid on to_submaps()
# ---------------------------------------------------------------------------------------------
E2E = [dict(name="force-fill", fill=True, lc=False), dict(name="radius-pools-no-radius", fill=False, lc=False), dict(name="force-fill-self", fill=True, lc=True)]


def e2e_maps(case):
    """Two maps of the same place of 60 segments each (cross pairs have true matches) — or, for self loop closures, ONE map of a
    loop of 30 segments driven twice (tests/_self_pools.two_lap_map: the second lap's segments carry their own ids)."""
    from roman_amd import synth
    import _self_pools as sp
    if case["lc"]:
        return [sp.two_lap_map(seed=61, n_lap=30)]
    maps = []
    for r in range(2):
        segs, traj, times = synth.make_map(60, D, seed=42, n_poses=60, dt=4.0)
        for q in segs:
            q.id = int(q.id) + 100000 * r
        maps.append((segs, traj, times))
    return maps


def e2e_params(case):
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    p = SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=case["fill"], submap_radius=15.0 if case["fill"] else None,
                          submap_max_size=12, submap_overlap=6, submap_center_dist=15.0, single_robot_lc=case["lc"], single_robot_lc_time_thresh=100.0)
    return p, sa.SubmapAlignIO(lc_association_thresh=4)


def run_e2e(case, ctx, device, fill_ctx=None, radius_ctx=None, compute=None):
    """-> (result of the pools path, result of the grid path, the pools, borderline flags of the boxes)."""
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import FillSubmapParams, MapTable, SubmapParams, build_submap_pool, fill_centers, submap_centers
    p, io = e2e_params(case)
    reg = p.get_object_registration(); reg.set_context(ctx)
    pools, segs = [], []
    for sg, traj, times in e2e_maps(case):
        table = MapTable.from_segments(reg, sg)
        if case["fill"]:
            fp = FillSubmapParams.from_submap_align_params(p)
            centers, slices = fill_centers(table, traj, times, fp)
            pool = build_submap_pool(reg, table, centers, fp, ctx=fill_ctx or ctx, device=device, fill=slices)
            want = fo.fill_oracle(table.feats, centers.descs(), slices, fp.max_size, seg_ids=table.ids)
            assert np.array_equal(pool.count, want["count"]) and np.array_equal(pool.src, want["src"])
            rows = pool.pool.cpu().numpy()
            for s in range(len(slices)):
                n = int(pool.count[s])
                assert rows[s * pool.cap:s * pool.cap + n].tobytes() == want["rows"][s].tobytes() and np.array_equal(pool.ids[s, :n], want["ids"][s])
            assert np.array_equal(pool.ids_dev.cpu().numpy(), pool.ids.reshape(-1))
        else:
            sp_ = SubmapParams(max_size=12, radius=15.0, distance=15.0, pruning_method='distance')
            pool = build_submap_pool(reg, table, submap_centers(traj, times, sp_), sp_, ctx=radius_ctx or ctx, device=device)
        pools.append(pool); segs.append(sg)
    if case["lc"]:
        pools, segs = [pools[0], pools[0]], [segs[0], segs[0]]
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pools, segs)], io, registration=reg, compute=compute)
    box = [fo.boxes_oracle(q.pool.cpu().numpy(), q.cap, q.count, q.centers.pose_flu)[q.nonempty] for q in pools]
    return got, want, pools, fo.borderline(box[0], box[1])


def check_e2e(case, got, want, flags):
    import _self_pools as sp
    assert flags == [], flags                                                # zero borderline pairs for the chosen seeds
    sp.compare(got, want)                                                    # (the tolerances of tests/test_gpu_submap_align_pools.py)
    n, near = want.clipper_num_associations, ~np.isnan(want.robots_nearby_mat)
    assert (n >= 4).sum() >= 2, "fewer than two pairs aligned: the comparison would show nothing"
    assert near.any() and (~near).any(), "every pair or no pair is nearby: the gate would show nothing"
    return dict(grid=n.shape, nearby=int(near.sum()), aligned=int((n >= 4).sum()), edges=len(want.lc_edges["pairs"]))


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for case in E2E:
        got, want, pools, flags = run_e2e(case, ctx, dev)
        print(f"{case['name']}: {check_e2e(case, got, want, flags)}")
    ctx.close()
    print("FILL_BOXES_OK")


@pytest.mark.gpu
def test_aabb_pools_path_equals_grid_path_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_fill_boxes as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FILL_BOXES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
