"""Frame-descriptor submaps on the device: roman_frame_select*, roman_stacked_sim*, roman_grid_gate_sim* against
tests/_frame_desc_oracle.py and tests/_grid_gate_oracle.py, and build_submap_pool(frames=...) -> submap_align_pools against
submap_align_grid on to_submaps() of the same pools, for the three descriptor modes.

Selections, counts, spans, flags and pair lists: exact.  Means and similarities: 1e-12 * max(1, |x|) (d-long sums whose order is
free in the contract, the tolerance of tests/test_gpu_grid_gate.py), and bit-identical between two calls and between band heights.
The case builders are shared with tests/test_frame_desc_cpu.py, which checks on the CPU that every seeded case is free of
borderline flags and that the end-to-end threshold splits the pairs."""
import subprocess
import sys

import numpy as np
import pytest

import _frame_desc_oracle as fo
import _grid_gate_oracle as go
from roman_amd import _abi
from roman_amd.runtime import frame_select_params, grid_gate_params

REL = 1e-12


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    inf = ~fin & ~np.isnan(want)
    return bool(np.array_equal(got[inf], want[inf]) and np.all(np.abs(got[fin] - want[fin]) <= REL * np.maximum(1.0, np.abs(want[fin]))))


# ---------------------------------------------------------------------------------------------
# frame_select: S = 6, cap = 8, N = 40, Nf = 70 (a second, partial mask word)
# ---------------------------------------------------------------------------------------------
S, CAP, N, NF = 6, 8, 40, 70
THIN = 2.5           # frames 1 m apart along a line: every third candidate is at least 2.5 m (3 m) from the last selected


def select_case(sorted_times=True, seed=11):
    """count, src, seg_times, frame_times, frame_pos.  Frame f has time 10 f + 5 (a permutation of that when not sorted) and sits
    at x = f (+- a seeded 0.05 m).  Submap 0: one segment whose span holds exactly one frame; 1: empty; 2: a span over every frame;
    3 - 5: seeded rows."""
    rng = np.random.default_rng(seed)
    ft = 10.0 * np.arange(NF) + 5.0
    if not sorted_times:
        ft = ft[rng.permutation(NF)]
    pos = np.stack([np.arange(NF) + rng.uniform(-0.05, 0.05, NF), rng.uniform(-0.05, 0.05, NF), rng.uniform(-0.02, 0.02, NF)], axis=1)
    first = rng.uniform(0.0, 10.0 * NF - 80.0, N); first = np.floor(first) + 0.25          # never within 1e-9 of a frame time (k + 0.25 vs 10 f + 5)
    seg = np.stack([first, first + np.floor(rng.uniform(10.0, 70.0, N)) + 0.5], axis=1)
    seg[0] = (122.0, 128.0)                                                                  # holds frame time 125 only
    seg[1] = (-3.0, 2.0); seg[2] = (690.0, 1000.0)                                           # together: every frame
    count = np.array([1, 0, 2, 8, 5, 3], dtype=np.int32)
    src = np.full((S, CAP), -1, dtype=np.int32)
    src[0, 0] = 0; src[2, :2] = (1, 2)
    for s in (3, 4, 5):
        src[s, :count[s]] = rng.choice(np.arange(3, N), count[s], replace=False)
    return dict(count=count, src=src, seg_times=seg, frame_times=ft, frame_pos=pos)


SELECT_CASES = [("all", True, None), ("thin", True, THIN), ("all-unsorted", False, None), ("thin-unsorted", False, THIN)]


def check_select_case(c, thin):
    """What the shapes are chosen for (checked on the CPU): no borderline flag, one-candidate / empty / whole-map submaps, and a
    thinning that keeps roughly every third candidate."""
    fo.clean(fo.borderline(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], thin), "select case")
    o = fo.frame_select_oracle(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], None, thin)
    assert len(o["cand"][0]) == 1 and o["n_sel"][0] == 1 and o["n_sel"][1] == 0 and len(o["cand"][2]) == NF
    assert np.isposinf(o["span"][1, 0]) and np.isneginf(o["span"][1, 1])
    assert o["mask"].shape == (S, 2) and (o["mask"][2, 1] >> np.uint64(NF - 64)) == 0
    if thin is not None:
        ratio = o["n_sel"][2:].sum() / sum(len(x) for x in o["cand"][2:])
        assert 0.2 < ratio < 0.5, ratio
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("name,sorted_times,thin", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
@pytest.mark.parametrize("d", [5, 16])
def test_frame_select_matches_the_oracle(ctx, name, sorted_times, thin, d):
    c = select_case(sorted_times)
    desc = np.random.default_rng(5).normal(0.0, 1.0, (NF, d))
    want = fo.frame_select_oracle(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], desc, thin, want_mean=True)
    check_select_case(c, thin)
    runs = [ctx.frame_select(frame_select_params(thin, True), c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], desc)
            for _ in range(2)]
    got = runs[0]
    assert np.array_equal(got.mask, want["mask"]) and np.array_equal(got.n_sel, want["n_sel"]) and np.array_equal(got.span, want["span"])
    for s in range(S):
        assert np.array_equal(got.selected(s), want["sel"][s])
    assert close(got.mean, want["mean"]) and np.isnan(got.mean[1]).all()
    assert np.array_equal(runs[0].mean.view(np.int64), runs[1].mean.view(np.int64)) and np.array_equal(runs[0].mask, runs[1].mask)
    # without the mean nothing of the descriptors is needed
    bare = ctx.frame_select(frame_select_params(thin, False), c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"])
    assert bare.mean is None and np.array_equal(bare.mask, want["mask"])


# ---------------------------------------------------------------------------------------------
# stacked_sim: Nf0 = 70, Nf1 = 37, S0 = 5, S1 = 7
# ---------------------------------------------------------------------------------------------
NF0, NF1, S0, S1 = 70, 37, 5, 7


def stacked_case(d, seed=23):
    """desc0, desc1, sel0, sel1.  Overlapping masks; sel0[1] one frame; sel0[3] empty; sel1[6] empty; frame 69 of map 0 has norm 0
    and sel0[4] = {69, 68} where frame 68 is the negative of a direction every frame of sel1[5] leans towards (all its cosines are
    negative: the zero-norm frame's 0 is the maximum); frames 0 .. 3 of map 1 are copies of frames 10 .. 13 of map 0."""
    rng = np.random.default_rng(seed + d)
    desc0 = rng.normal(0.0, 1.0, (NF0, d)); desc1 = rng.normal(0.0, 1.0, (NF1, d))
    desc1[:4] = desc0[10:14]
    lean = np.abs(rng.normal(0.0, 1.0, d)) + 0.5
    desc1[30:36] = lean + 0.05 * rng.normal(0.0, 1.0, (6, d))
    desc0[68] = -lean; desc0[69] = 0.0
    sel0 = [np.arange(0, 40), np.array([12]), np.arange(20, 70, 3), np.array([], dtype=np.int64), np.array([68, 69])]
    sel1 = [np.arange(0, 20), np.arange(10, 37), np.array([2]), np.arange(5, 30, 2), np.arange(0, 37), np.arange(30, 36), np.array([], dtype=np.int64)]
    return desc0, desc1, sel0, sel1


def check_stacked_case(d):
    desc0, desc1, sel0, sel1 = stacked_case(d)
    fo.clean(fo.borderline_sim(desc0, sel0, desc1, sel1), f"stacked case d={d}")
    want = fo.stacked_sim_oracle(desc0, sel0, desc1, sel1)
    assert np.isneginf(want[3]).all() and np.isneginf(want[:, 6]).all() and np.isfinite(np.delete(np.delete(want, 3, 0), 6, 1)).all()
    assert want[4, 5] == 0.0, want[4, 5]                                    # the zero-norm frame among negative cosines
    assert abs(want[1, 2] - 1.0) <= REL and abs(want[0, 0] - 1.0) <= REL      # identical frames on both sides
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 19, 64])
def test_stacked_sim_matches_the_oracle_at_every_band_height(ctx, d):
    desc0, desc1, sel0, sel1 = stacked_case(d)
    want = check_stacked_case(d)
    m0, m1 = fo.pack_mask(sel0, NF0), fo.pack_mask(sel1, NF1)
    try:
        runs = [ctx.stacked_sim(desc0, m0, desc1, m1) for _ in range(2)]
        ctx.set_stacked_band(_abi.STACKED_BAND_MIN)                         # 70 frames: three bands
        banded = ctx.stacked_sim(desc0, m0, desc1, m1)
    finally:
        ctx.set_stacked_band(0)
    assert close(runs[0], want), (runs[0], want)
    assert runs[0][4, 5] == 0.0
    assert np.array_equal(runs[0].view(np.int64), runs[1].view(np.int64))
    assert np.array_equal(runs[0].view(np.int64), banded.view(np.int64))
    # the transposed problem: 37 rows against 70 columns
    assert close(ctx.stacked_sim(desc1, m1, desc0, m0), want.T)


@pytest.mark.gpu
def test_stacked_sim_degenerate_shapes(ctx):
    desc0, desc1, sel0, sel1 = stacked_case(3)
    m0, m1 = fo.pack_mask(sel0, NF0), fo.pack_mask(sel1, NF1)
    assert ctx.stacked_sim(desc0, m0[:0], desc1, m1).shape == (0, S1)
    none = ctx.stacked_sim(desc0[:0], np.zeros((S0, 0), np.uint64), desc1, m1)
    assert none.shape == (S0, S1) and np.isneginf(none).all()


# ---------------------------------------------------------------------------------------------
# grid_gate_sim on a clean 5 x 7 grid
# ---------------------------------------------------------------------------------------------
GATE = dict(radius=12.0, skip_distance=35.0, desc_thresh=0.45, single_robot_lc=True, lc_time_thresh=60.0)


def gate_case():
    """A clean seeded grid with vector descriptors (d = 2 unit vectors: |a| = |b| = 1 up to rounding) and the similarity the
    existing gate computes from them on the oracle."""
    a, b = go.clean_grid(77, S0, S1, 2, **GATE)
    for side in (a, b):
        ang = np.random.default_rng(len(side["pos"])).uniform(0.0, np.pi, len(side["pos"]))
        side["desc"] = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    assert not go.borderline(a, b, **GATE)
    o = go.grid_gate_oracle(a, b, **GATE)
    f = o["flags"]
    assert ((f & go.SKIP) != 0).any() and ((f & go.GATED) != 0).any() and ((f & go.TODO) != 0).any()
    return a, b, o


@pytest.mark.gpu
def test_grid_gate_sim_equals_the_gate_fed_descriptors(ctx):
    a, b, _ = gate_case()
    with_desc = ctx.grid_gate(grid_gate_params(GATE["radius"], GATE["skip_distance"], 2, GATE["desc_thresh"], True, GATE["lc_time_thresh"]),
                              a["pos"], a["T_w"], b["pos"], b["T_w"], a["time"], b["time"], a["desc"], b["desc"])
    sim = with_desc.sim.copy()
    keep = sim.copy()
    got = ctx.grid_gate_sim(grid_gate_params(GATE["radius"], GATE["skip_distance"], 0, GATE["desc_thresh"], True, GATE["lc_time_thresh"]),
                            sim, a["pos"], a["T_w"], b["pos"], b["T_w"], a["time"], b["time"])
    assert np.array_equal(sim.view(np.int64), keep.view(np.int64)), "sim was written"
    assert got.n_todo == with_desc.n_todo and 0 < got.n_todo < S0 * S1
    assert np.array_equal(got.flags, with_desc.flags) and np.array_equal(got.pairs, with_desc.pairs) and np.array_equal(got.enable, with_desc.enable)
    for name in ("dist", "yaw_deg", "T_ij", "T_ref"):
        assert np.array_equal(getattr(got, name).view(np.int64), getattr(with_desc, name).view(np.int64)), name
    with pytest.raises(_abi.RomanHipError) as e:
        ctx.grid_gate_sim(grid_gate_params(GATE["radius"], GATE["skip_distance"], 2, GATE["desc_thresh"]), sim, a["pos"], a["T_w"], b["pos"], b["T_w"])
    assert e.value.code == _abi.ROMAN_E_INVALID


@pytest.mark.gpu
def test_argument_checks(ctx):
    """Every ROMAN_E_* case of the three contracts, through the real library's checks on a real context (a NULL context returns
    before them: tests/test_frame_desc_abi.py)."""
    import ctypes as C
    lib, h = ctx._lib, ctx._h
    buf = np.zeros(64, np.int64)
    v = C.c_void_p(buf.ctypes.data)                               # never dereferenced: every call below fails its checks
    sel = lambda P, S=1, cap=1, N=1, Nf=1, d=1, desc=v, ft=v, fpos=v, mask=v, mean=v: lib.roman_frame_select_dev(
        h, C.byref(P), S, cap, v, v, N, v, Nf, ft, fpos, d, desc, mask, v, v, mean)
    bad = frame_select_params(1.0, False); bad.reserved[1] = 1
    for P, kw in ((frame_select_params(float("nan")), {}), (frame_select_params(-1.0), {}), (bad, {}), (frame_select_params(None, True), dict(d=0)),
                  (frame_select_params(None, True), dict(desc=None)), (frame_select_params(), dict(S=-1)), (frame_select_params(), dict(Nf=-1)),
                  (frame_select_params(), dict(cap=0)), (frame_select_params(), dict(ft=None)), (frame_select_params(2.0), dict(fpos=None)),
                  (frame_select_params(), dict(mask=None)), (frame_select_params(None, True), dict(mean=None))):
        assert sel(P, **kw) == _abi.ROMAN_E_INVALID, kw
    assert sel(frame_select_params(), S=0) == _abi.ROMAN_OK and sel(frame_select_params(), S=0, Nf=0) == _abi.ROMAN_OK
    sim = lambda d=4, Nf0=1, S0=1, Nf1=1, S1=1, desc0=v, out=v: lib.roman_stacked_sim_dev(h, d, Nf0, desc0, S0, v, Nf1, v, S1, v, out)
    assert sim(d=0) == _abi.ROMAN_E_INVALID and sim(Nf0=-1) == _abi.ROMAN_E_INVALID and sim(desc0=None) == _abi.ROMAN_E_INVALID
    assert sim(out=None) == _abi.ROMAN_E_INVALID and sim(S0=70000, S1=70000) == _abi.ROMAN_E_TOO_LARGE
    assert sim(S0=0) == _abi.ROMAN_OK and sim(S1=0, out=None) == _abi.ROMAN_OK
    with pytest.raises(_abi.RomanHipError):
        ctx.set_stacked_band(-1)
    ctx.sync()


# ---------------------------------------------------------------------------------------------
# end to end: two maps -> build_submap_pool(frames=...) x 2 -> submap_align_pools, against submap_align_grid on to_submaps()
# ---------------------------------------------------------------------------------------------
D = 16
# the thresholds sit in gaps of the similarities of these maps (tests/test_frame_desc_cpu.py checks on the CPU that the nearest
# similarity lies more than 1e-6 away and that either side of the threshold holds pairs)
E2E = [dict(name="mean", mode='mean_frame_descriptor', dist=None, thresh=0.90),
       dict(name="stacked-all", mode='stacked_frame_descriptors', dist=None, thresh=0.97),
       dict(name="stacked-10m", mode='stacked_frame_descriptors', dist=10.0, thresh=0.95)]


def e2e_maps():
    """The same place mapped twice (cross pairs have true matches): 120 segments, 30 frames; the second robot's frame descriptors
    are the first's plus seeded noise, so submaps that see the same stretch of the path are similar and others are not."""
    from roman_amd import synth
    from roman_amd.align.submaps import FrameTable
    base = fo.frame_descriptors(np.random.default_rng(900), 30, D, walk=0.6)
    maps = []
    for r in range(2):
        segs, traj, times = synth.make_map(120, D, seed=41, n_poses=30, dt=8.0)
        if r == 1:
            for q in segs:
                q.id = int(q.id) + 100000
        desc = base + (0.15 * np.random.default_rng(901).normal(0.0, 1.0, base.shape) if r else 0.0)
        maps.append((segs, traj, times, FrameTable.from_map(traj, times, list(desc))))
    return maps


def run_e2e(case, ctx, device, build_ctx=None, compute=None):
    """-> (result of the pools path, result of the grid path, the pools)."""
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=20.0, submap_max_size=40, submap_center_time=50.0,
                          submap_descriptor=case["mode"], frame_descriptor_dist=case["dist"], submap_descriptor_thresh=case["thresh"])
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = p.get_object_registration()
    params = SubmapParams.from_submap_align_params(p)
    pools, segs = [], []
    for sg, traj, times, frames in e2e_maps():
        table = MapTable.from_segments(reg, sg)
        pools.append(build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=build_ctx or ctx, device=device, frames=frames))
        segs.append(sg)
    reg.set_context(ctx(pools) if callable(ctx) else ctx)      # (a stand-in context is sized by the pools it will view)
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pools, segs)], io, registration=reg, compute=compute)
    return got, want, pools


def compare_e2e(case, got, want, margin=1e-6):
    n = want.clipper_num_associations
    sim = want.similarity_mat
    assert sim is not None and got.similarity_mat is not None
    assert np.nanmin(np.abs(sim - case["thresh"])) > margin, "a similarity sits on the threshold: choose another"
    assert (sim < case["thresh"]).any() and (sim >= case["thresh"]).any(), "the threshold does not split the pairs"
    assert np.array_equal(got.clipper_num_associations, n, equal_nan=True)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    for i in range(n.shape[0]):
        for j in range(n.shape[1]):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert (n >= 4).sum() >= 2, "hardly a pair of the grid aligned: the comparison would show nothing"
    for name in ("T_ij_mat", "T_ij_hat_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
    for name in ("clipper_angle_mat", "clipper_dist_mat", "submap_yaw_diff_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    np.testing.assert_allclose(got.similarity_mat, sim, rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"]) and len(want.lc_edges["pairs"]) >= 2
    np.testing.assert_allclose(got.lc_edges["t"], want.lc_edges["t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.lc_edges["q"], want.lc_edges["q"], rtol=0, atol=1e-12)


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    for case in E2E:
        got, want, pools = run_e2e(case, ctx, dev)
        compare_e2e(case, got, want)
        print(f"{case['name']}: {want.clipper_num_associations.shape} grid, {len(got.timing_list)} pairs registered, "
              f"{len(want.lc_edges['pairs'])} loop closures, frames per submap {[int(x) for x in pools[0].frame_n]}")
    ctx.close()
    print("FRAME_DESC_OK")


@pytest.mark.gpu
def test_pools_path_equals_grid_path_for_the_frame_descriptor_modes():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_frame_desc as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FRAME_DESC_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
