"""Pass 1 of the grid on the device without a GPU: the NumPy restatement of roman_grid_gate's contract
(tests/_grid_gate_oracle.py) against pass 1 of submap_align_grid, the entry points at the C-ABI boundary, and submap_align_pools
over a stand-in context against submap_align_grid on the same pools' to_submaps()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _grid_gate_oracle as go
import _lc_tail
from _stub_context import OracleContext, _view
from conftest import ROOT
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.runtime import LcInputs, LoopClosureResult, lc_record_dtype, stats_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_grid_gate_dev", "roman_grid_gate")
REL = 1e-12


def close(got, want):
    """|got - want| <= 1e-12 * max(1, |want|), NaN exactly where want has NaN, infinities equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    return bool(np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
                and np.all(np.abs(got[fin] - want[fin]) <= REL * np.maximum(1.0, np.abs(want[fin]))))


# ---------------------------------------------------------------------------------------------
# the oracle against pass 1 of submap_align_grid
# ---------------------------------------------------------------------------------------------
def _submaps_of(side, rng, use_desc):
    out = []
    for s in range(len(side["pos"])):
        gt = None if side["pos_gt"] is None else go.yaw_pose(rng.uniform(-np.pi, np.pi), side["pos_gt"][s])
        segs = [_lc_tail._Seg(1000 * s + q) for q in range(2)]
        out.append(sa.Submap(id=s, time=float(side["time"][s]), segments=segs, pose_flu=side["T_w"][s].copy(), pose_flu_gt=gt,
                             descriptor=side["desc"][s].copy() if use_desc else None))
    return out


def _failing_compute(seen):
    """compute double: every registered pair fails for want of associations; remembers the pairs in the order they came."""
    def compute(registration, batch, lc):
        B = len(batch)
        seen.append(np.array(batch.pair_index))
        status = np.full(B, _abi.ROMAN_ST_INSUFFICIENT, dtype=np.int32)
        rec, acc = _lc_tail.lc_tail(lc, np.full((B, 4, 4), np.nan), np.zeros(B, np.int32), status)
        return LoopClosureResult([np.zeros((0, 2), np.int32)] * B, np.full((B, 4, 4), np.nan), status, np.zeros(B, stats_dtype()), rec, acc)
    return compute


GRID_CASES = [dict(seed=s, skip=skip, d=d, gt=gt, lc=lc)
              for s, (skip, d, gt, lc) in enumerate([(np.inf, 0, (False, False), False), (25.0, 0, (True, False), True), (np.inf, 16, (False, True), False),
                                                     (25.0, 16, (True, True), True), (40.0, 7, (False, False), True), (np.inf, 33, (True, True), False)])]


@pytest.mark.parametrize("case", GRID_CASES, ids=[f"skip{c['skip']}-d{c['d']}-gt{int(c['gt'][0])}{int(c['gt'][1])}" for c in GRID_CASES])
def test_oracle_equals_pass_1_of_submap_align_grid(case):
    d, gt = case["d"], case["gt"]
    gate = dict(radius=12.0, skip_distance=case["skip"], desc_thresh=0.6 if d else 0.0, single_robot_lc=case["lc"], lc_time_thresh=60.0)
    a, b = go.clean_grid(500 + case["seed"], 7, 9, max(d, 1), gt=gt, **gate)
    if d == 0:
        a["desc"] = b["desc"] = None
    rng = np.random.default_rng(case["seed"])
    S = [_submaps_of(a, rng, d > 0), _submaps_of(b, rng, d > 0)]
    # the sides as the caller of the device call resolves them: ground truth for the reference transform where it is available
    for side, sms, has in ((a, S[0], gt[0]), (b, S[1], gt[1])):
        side["T_w"] = np.stack([sa.transform_rm_roll_pitch(np.array(sm.pose_flu_gt if has else sm.pose_flu)) for sm in sms])
    o = go.grid_gate_oracle(a, b, **gate)
    p = SubmapAlignParams(submap_radius=gate["radius"], submap_descriptor='mean_semantic' if d else None, submap_descriptor_thresh=gate["desc_thresh"],
                          single_robot_lc=False)
    io = sa.SubmapAlignIO(skip_distance=case["skip"], gt_available=gt)
    seen = []
    res = sa.submap_align_grid(p, S, io, registration=_lc_tail.StubRegistration(3, False), compute=_failing_compute(seen))
    nearby = (o["flags"] & go.NEARBY) != 0
    todo = (o["flags"] & go.TODO) != 0
    assert 0 < nearby.sum() < nearby.size and 0 < todo.sum() and (d == 0 or todo.sum() < (~((o["flags"] & go.SKIP) != 0)).sum())
    assert np.array_equal(np.where(nearby, o["dist"], np.nan), res.robots_nearby_mat, equal_nan=True)      # exact
    assert len(seen) == 1 and np.array_equal(seen[0], o["pairs"])                                          # the todo set and its order
    assert o["n_todo"] == len(o["pairs"]) and np.array_equal(o["T_ref"], o["T_ij"][o["pairs"][:, 0], o["pairs"][:, 1]])
    assert close(o["T_ij"], res.T_ij_mat)
    assert close(o["yaw_deg"], res.submap_yaw_diff_mat)
    if d:
        skip = (o["flags"] & go.SKIP) != 0
        assert close(np.where(skip, np.nan, o["sim"]), res.similarity_mat)
        assert np.array_equal((o["flags"] & go.GATED) != 0, ~skip & ~todo)
    else:
        assert res.similarity_mat is None and np.isposinf(o["sim"]).all()
    # the time gate, against the expression of submap_align_grid
    dt = np.abs(a["time"][o["pairs"][:, 0]] - b["time"][o["pairs"][:, 1]])
    assert np.array_equal(o["enable"], np.where(case["lc"] & (dt < 60.0), 0, 1))
    assert not case["lc"] or 0 < o["enable"].sum() < len(o["enable"])


def test_borderline_detector_flags_what_it_should():
    gate = dict(radius=10.0, skip_distance=30.0, desc_thresh=0.5, single_robot_lc=True, lc_time_thresh=60.0)
    a, b = go.clean_grid(3, 4, 5, 8, **gate)
    assert not go.borderline(a, b, **gate)
    for shift, msg in ((20.0 + 5e-10, "radius"), (30.0 - 5e-10, "skip")):
        b2 = dict(b); b2["pos"] = b["pos"].copy(); b2["pos"][2] = a["pos"][1] + np.array([shift, 0.0, 0.0])
        assert go.borderline(a, b2, **gate), msg
    b2 = dict(b); b2["time"] = b["time"].copy(); b2["time"][0] = a["time"][3] + 60.0 + 3e-10
    assert go.borderline(a, b2, **gate) and not go.borderline(a, b2, **{**gate, "single_robot_lc": False})
    o = go.grid_gate_oracle(a, b, **gate)
    assert go.borderline(a, b, **{**gate, "desc_thresh": float(o["sim"][1, 1]) + 4e-10})
    a2 = dict(a); a2["desc"] = a["desc"].copy(); a2["desc"][0] = 0.0; a2["desc"][0, 0] = 1e-9 / np.linalg.norm(b["desc"][0])
    assert go.borderline(a2, b, **gate)
    with pytest.raises(AssertionError):
        go.clean_grid(3, 4, 5, 8, **{**gate, "desc_thresh": float(o["sim"][1, 1]) + 4e-10})


# ---------------------------------------------------------------------------------------------
# the C-ABI boundary
# ---------------------------------------------------------------------------------------------
def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == 23, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == 23, s
        assert "[REF roman/align/submap_align.py:93-149]" in src[max(0, at - 4000):at], s       # the comment above cites what it replaces
    for name in ("NEARBY", "SKIP", "GATED", "TODO"):
        assert f"#define ROMAN_GRID_{name}" in src and getattr(_abi, f"ROMAN_GRID_{name}") == getattr(go, name)


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.RomanGridGateParams._fields_]
    assert fields == ["radius", "skip_distance", "desc_dim", "reserved0", "desc_thresh", "single_robot_lc", "reserved1", "lc_time_thresh", "reserved"]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(roman_grid_gate_params_t, {f}));' for f in fields)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof %zu\\n", sizeof(roman_grid_gate_params_t));\n{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == C.sizeof(_abi.RomanGridGateParams) == _abi.GRID_GATE_PARAMS_NBYTES == 56
    for f in fields:
        assert int(out[f]) == getattr(_abi.RomanGridGateParams, f).offset, f


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    from roman_amd.runtime import grid_gate_params
    P = grid_gate_params(5.0)
    n = np.zeros(4, np.int64)
    v = C.c_void_p(n.ctypes.data)
    for fn in (lib.roman_grid_gate_dev, lib.roman_grid_gate):
        assert fn(None, C.byref(P), 0, 0, *([None] * 10), *([v] * 9)) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)


# ---------------------------------------------------------------------------------------------
# submap_align_pools over a stand-in context
# ---------------------------------------------------------------------------------------------
class PoolsStubContext(OracleContext):
    """tests/_stub_context.OracleContext (the batch call through the CPU oracle) plus the two calls submap_align_pools adds: the
    gate through tests/_grid_gate_oracle.py and the tail through tests/_lc_tail.py, both written through the raw addresses."""

    def __init__(self, n_objects, dim=3):
        super().__init__(n_objects, dim)
        self.gates, self.tails, self.order = 0, 0, []

    def align_batch_dev(self, *a, **kw):
        self.order.append("batch")
        return super().align_batch_dev(*a, **kw)

    def grid_gate_dev(self, gp, S0, S1, pos0, T_w0, pos1, T_w1, dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, n_todo,
                      time0_ptr=None, time1_ptr=None, desc0_ptr=None, desc1_ptr=None, pos_gt0_ptr=None, pos_gt1_ptr=None):
        self.gates += 1; self.order.append("gate")
        assert gp.radius >= 0 and not any((gp.reserved0, gp.reserved1, gp.reserved[0], gp.reserved[1]))
        d = int(gp.desc_dim)
        side = lambda S, pos, gt, T, tm, desc: dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(gt, (S, 3), np.float64) if gt else None,
                                                    T_w=_view(T, (S, 4, 4), np.float64), time=_view(tm, (S,), np.float64),
                                                    desc=_view(desc, (S, d), np.float64) if d else None)
        o = go.grid_gate_oracle(side(S0, pos0, pos_gt0_ptr, T_w0, time0_ptr, desc0_ptr), side(S1, pos1, pos_gt1_ptr, T_w1, time1_ptr, desc1_ptr),
                                gp.radius, gp.skip_distance, gp.desc_thresh, bool(gp.single_robot_lc), gp.lc_time_thresh)
        B = S0 * S1
        _view(dist, (S0, S1), np.float64)[:] = o["dist"]; _view(flags, (S0, S1), np.int32)[:] = o["flags"]
        _view(yaw, (S0, S1), np.float64)[:] = o["yaw_deg"]; _view(sim, (S0, S1), np.float64)[:] = o["sim"]
        _view(T_ij, (S0, S1, 4, 4), np.float64)[:] = o["T_ij"]
        n = o["n_todo"]
        _view(pairs, (B, 2), np.int32)[:n] = o["pairs"]; _view(T_ref, (B, 4, 4), np.float64)[:n] = o["T_ref"]
        _view(enable, (B,), np.int32)[:n] = o["enable"]; _view(n_todo, (1,), np.int32)[0] = n

    def lc_tail_dev(self, lp, B, T_ptr, n_ptr, st_ptr, rec_ptr, idx_ptr, cnt_ptr, T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None,
                    FR_ptr=None, iR_ptr=None):
        self.tails += 1; self.order.append("tail")
        s = int(lp.dim) + 1
        iL, iR = _view(iL_ptr, (B,), np.int32), _view(iR_ptr, (B,), np.int32)
        lc = LcInputs(dim=int(lp.dim), force_rm_upside_down=bool(lp.force_rm_upside_down), force_rm_lc_roll_pitch=bool(lp.force_rm_lc_roll_pitch),
                      tilt_thresh=None if lp.tilt_thresh < 0 else float(lp.tilt_thresh), lc_association_thresh=int(lp.lc_association_thresh),
                      T_ref=_view(T_ref_ptr, (B, 4, 4), np.float64), enable=_view(enable_ptr, (B,), np.int32),
                      FL=_view(FL_ptr, (int(iL.max()) + 1, 4, 4), np.float64), iL=iL, FR=_view(FR_ptr, (int(iR.max()) + 1, 4, 4), np.float64), iR=iR)
        rec, acc = _lc_tail.lc_tail(lc, _view(T_ptr, (B, 16), np.float64)[:, :s * s].reshape(B, s, s), _view(n_ptr, (B,), np.int32), _view(st_ptr, (B,), np.int32))
        _view(rec_ptr, (B,), lc_record_dtype())[:] = rec
        _view(idx_ptr, (B,), np.int32)[:len(acc)] = acc; _view(cnt_ptr, (1,), np.int32)[0] = len(acc)


D = 16


def _pools(method="roman", descriptor='mean_semantic', seeds=(31, 31), shift=(0.0, 0.0, 0.0), dim=3, id_offset=100000):
    import _submaps_oracle as so
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    reg = SubmapAlignParams(method=method, semantics_dim=D, dim=dim).get_object_registration()
    params = SubmapParams(max_size=12, radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor=descriptor)
    pools, segs = [], []
    for r, seed in enumerate(seeds):
        sg, traj, times = synth.make_map(90, D, seed=seed, n_poses=24, dt=8.0)
        if r == 1:
            for q in sg:
                q.id = int(q.id) + id_offset                   # another robot's map: its own segment ids
        table = MapTable.from_segments(reg, sg)
        pools.append(build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=so.OracleSubmapContext(), device="cpu"))
        segs.append(sg)
    reg.set_context(PoolsStubContext(int(pools[0].pool.shape[0] + pools[1].pool.shape[0]), dim))
    return reg, pools, segs


def assert_same_results(got, want):
    for name in ("robots_nearby_mat", "clipper_num_associations"):
        assert np.array_equal(getattr(got, name), getattr(want, name), equal_nan=True), name
    for name in ("T_ij_mat", "T_ij_hat_mat", "submap_yaw_diff_mat"):
        assert close(getattr(got, name), getattr(want, name)), name
    for name in ("clipper_angle_mat", "clipper_dist_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    assert (got.similarity_mat is None) == (want.similarity_mat is None)
    if want.similarity_mat is not None:
        assert close(got.similarity_mat, want.similarity_mat)
    n0, n1 = want.robots_nearby_mat.shape
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
    assert close(got.lc_edges["t"], want.lc_edges["t"]) and close(got.lc_edges["q"], want.lc_edges["q"])


@pytest.mark.parametrize("kind", ["roman-descriptor", "gravity-skip", "single-robot-times"])
def test_pools_path_equals_grid_path_on_a_stand_in(kind):
    if kind == "roman-descriptor":
        reg, pools, segs = _pools("roman", 'mean_semantic')
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8)
        io = sa.SubmapAlignIO(lc_association_thresh=4)
    elif kind == "gravity-skip":
        reg, pools, segs = _pools("gravity", None)
        p = SubmapAlignParams(method="gravity", semantics_dim=D, submap_radius=15.0)
        io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=35.0)
    else:
        reg, pools, segs = _pools("roman", None)
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
        io = sa.SubmapAlignIO(lc_association_thresh=4)
    ctx = reg._context()
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    assert ctx.gates == 1 and ctx.tails == 1 and ctx.order[0] == "gate" and ctx.order[-1] == "tail" and "batch" in ctx.order
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pools, segs)], io, registration=reg, compute=_lc_tail.oracle_lc_compute)
    assert_same_results(got, want)
    n = want.clipper_num_associations
    assert (n >= 4).sum() >= 2, "no pair of the grid aligned: the comparison would show nothing"
    if kind == "roman-descriptor":
        done = ~np.isnan(want.T_ij_hat_mat[:, :, 0, 0])
        assert done.any() and (want.similarity_mat < 0.8).any() and (want.similarity_mat >= 0.8).any()
    if kind == "gravity-skip":
        assert np.isnan(want.similarity_mat if want.similarity_mat is not None else np.nan).all()
        assert (n == 0).any() and len(got.timing_list) < n.size                       # some pairs were skipped for distance
    if kind == "single-robot-times":
        assert len(want.lc_edges["pairs"]) < (n >= 4).sum(), "the time gate disabled no accepted pair"


def test_pools_path_refuses_what_it_does_not_cover():
    reg, pools, segs = _pools("roman", 'mean_semantic')
    io = sa.SubmapAlignIO()
    base = dict(method="roman", semantics_dim=D, submap_radius=15.0)
    way = "to_submaps"
    cases = [
        (SubmapAlignParams(**base, single_robot_lc=True), (pools[0], pools[0]), reg),
        (SubmapAlignParams(**base, force_fill_submaps=True), pools, reg),
        (SubmapAlignParams(**{**base, "submap_radius": None}), pools, reg),
        (SubmapAlignParams(**base, submap_descriptor='stacked_frame_descriptors'), pools, reg),
        (SubmapAlignParams(**base, submap_descriptor='mean_frame_descriptor'), pools, reg),
        (SubmapAlignParams(**{**base, "method": "ransac"}), pools, SubmapAlignParams(method="ransac").get_object_registration()),
        (SubmapAlignParams(**{**base, "method": "clipper+prune"}), pools, SubmapAlignParams(method="clipper+prune", semantics_dim=D).get_object_registration()),
    ]
    for p, pl, r in cases:
        with pytest.raises(ValueError, match=way) as e:
            sa.submap_align_pools(p, pl, io, registration=r)
        assert "submap_align_grid" in str(e.value)
    assert reg._context().gates == 0
    # single_robot_lc over two pools of the SAME map (shared segment ids) is refused too; over maps with their own ids it runs
    _, same, _ = _pools("roman", None, id_offset=0)
    with pytest.raises(ValueError, match=way):
        sa.submap_align_pools(SubmapAlignParams(**base, single_robot_lc=True), same, io, registration=reg)
    # a pool built without descriptors cannot serve the descriptor gate
    _, bare, _ = _pools("roman", None)
    with pytest.raises(ValueError, match="mean_semantic"):
        sa.submap_align_pools(SubmapAlignParams(**base, submap_descriptor='mean_semantic'), bare, io, registration=reg)


def test_submap_align_grid_still_fills_its_results_through_the_shared_helper():
    """The block both functions call: submap_align_grid's results on the planted cases of tests/_lc_tail.py are what the per-pair
    code gives (tests/test_lc_tail_cpu.py checks the same through the records)."""
    case = _lc_tail.make_cases(**_lc_tail.ALL_CASES[0])
    p, io, reg = _lc_tail.case_params(case)
    import copy

    def compute(registration, batch, lc):
        from roman_amd.runtime import BatchResult
        B = case["B"]
        assoc = [np.zeros((int(case["n_assoc"][b]), 2), np.int32) for b in range(B)]
        return _lc_tail.as_lc_result(BatchResult(assoc, case["T"].copy(), case["status"].copy(), np.zeros(B, stats_dtype())), lc)
    res = sa.submap_align_grid(p, copy.deepcopy(case["submaps"]), io, registration=reg, compute=compute)
    _, _, want = _lc_tail.per_pair_reference(case)
    assert np.array_equal(res.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
    np.testing.assert_allclose(res.T_ij_hat_mat, want.T_ij_hat_mat, rtol=0, atol=1e-8, equal_nan=True)
    np.testing.assert_allclose(res.clipper_dist_mat, want.clipper_dist_mat, rtol=0, atol=1e-7, equal_nan=True)
