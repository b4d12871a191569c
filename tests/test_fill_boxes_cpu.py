"""Force-fill submaps, the boxes of a pool and the bounding-box gate without a GPU: `fill_centers` and the NumPy
restatement (tests/_fill_boxes_oracle.py) against the reference's own results (tests/golden/fill_golden.npz), submap_align_pools
in AABB mode over a stand-in context against submap_align_grid on the same pools' to_submaps(), and the entry points at the
C-ABI boundary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _fill_boxes_oracle as fo
import _lc_tail
import _submaps_oracle as so
import test_grid_gate_cpu as gg
from _stub_context import _view
from conftest import ROOT
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import FillSubmapParams, MapTable, SubmapParams, build_submap_pool, fill_centers, submap_centers

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
# name -> number of arguments
ENTRY_POINTS = {"roman_submaps_fill_dev": 15, "roman_submaps_fill": 15, "roman_submap_boxes_dev": 8, "roman_submap_boxes": 8,
                "roman_grid_gate_aabb_dev": 26, "roman_grid_gate_aabb": 26}
D = 16
GOLDEN = fo.golden_cases()


# ---------------------------------------------------------------------------------------------
# the restatement and fill_centers against the reference's own results
# ---------------------------------------------------------------------------------------------
def _table(case):
    return MapTable(case["feats"], case["times"], case["ids"], 3, D)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_fill_centers_equals_the_reference(case):
    assert case["n_borderline"] == 0                                         # the committed fixture holds unambiguous cases only
    table = _table(case)
    before = case["trajectory"].copy()
    centers, slices = fill_centers(table, list(case["trajectory"]), case["traj_times"], FillSubmapParams(case["max_size"], case["overlap"]))
    assert np.array_equal(before, case["trajectory"])                        # the caller's trajectory is not flattened
    assert len(slices) == len(case["src"]) == len(centers)
    for got, want in zip(slices, case["src"]):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(centers.time, case["sm_time"]) and np.array_equal(centers.index, case["sm_index"])
    o_sl, mean, o_idx = fo.fill_slices(case["times"], case["traj_times"], case["max_size"], case["overlap"])
    assert all(np.array_equal(a, b) for a, b in zip(o_sl, slices)) and np.array_equal(o_idx, centers.index)
    assert not fo.borderline(slice_mean=mean, traj_times=case["traj_times"])
    # the pool through the stand-in gather: centres to 1e-12 (the reference multiplies with a matrix-vector product), descriptors too
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    ctx = fo.OracleFillContext()
    pool = build_submap_pool(reg, table, centers, FillSubmapParams(case["max_size"], case["overlap"], 'mean_semantic'), ctx=ctx, device="cpu", fill=slices)
    assert ctx.calls == 1 and pool.cap == case["max_size"]
    rows = pool.pool.numpy()
    for s, (src, cen) in enumerate(zip(case["src"], case["cen"])):
        n = len(src)
        assert pool.count[s] == n and np.array_equal(pool.src[s, :n], src) and np.all(pool.src[s, n:] == -1)
        assert np.array_equal(pool.ids[s, :n], case["ids"][src])
        np.testing.assert_allclose(rows[s * pool.cap:s * pool.cap + n, :3], cen, rtol=0, atol=1e-12)
        assert np.array_equal(rows[s * pool.cap:s * pool.cap + n, 3:], case["feats"][src, 3:])           # the other columns bit for bit
    np.testing.assert_allclose(pool.desc, case["sm_desc"], rtol=0, atol=1e-12)
    # boxes and the six comparisons against the reference's aabb_intersects over segments_as_global_points
    box = fo.boxes_oracle(rows, pool.cap, pool.count, centers.pose_flu)
    assert not fo.borderline(box, box)
    assert np.array_equal(fo.aabb_nearby(box, box), case["nearby"])


def test_fill_centers_shapes_and_refusals():
    case = GOLDEN[0]
    table = _table(case)
    traj, tt = list(case["trajectory"]), case["traj_times"]
    N = len(table)
    for max_size, overlap, S in ((8, 3, -(-N // 5)), (8, 0, N // 8), (N + 5, 2, 1)):
        centers, slices = fill_centers(table, traj, tt, FillSubmapParams(max_size, overlap))
        assert len(slices) == S and all(len(s) == min(max_size, N - i * (max_size - overlap)) for i, s in enumerate(slices))
        assert np.all(np.isneginf(centers.t_lo)) and np.all(np.isposinf(centers.t_hi))
        for T, Ti in zip(centers.pose_flu, centers.T_center_odom):            # flattened copies with their inverses
            assert abs(T[2, 0]) + abs(T[2, 1]) + abs(T[0, 2]) + abs(T[1, 2]) == 0.0 and np.allclose(T @ Ti, np.eye(4), atol=1e-12)
    for max_size, overlap in ((8, 8), (8, 9)):                               # range() with a step < 1
        with pytest.raises(ValueError):
            fill_centers(table, traj, tt, FillSubmapParams(max_size, overlap))
    empty = MapTable(case["feats"][:0], case["times"][:0], case["ids"][:0], 3, D)
    centers, slices = fill_centers(empty, traj, tt, FillSubmapParams(8, 3))
    assert len(centers) == 0 and slices == []
    # exact ties keep map order (Python's stable sorted())
    tied = MapTable(case["feats"][:6], np.tile(case["times"][:1], (6, 1)), case["ids"][:6], 3, D)
    _, slices = fill_centers(tied, traj, tt, FillSubmapParams(4, 2))
    assert [s.tolist() for s in slices] == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5]]


def test_fill_params_from_submap_align_params():
    p = FillSubmapParams.from_submap_align_params(SubmapAlignParams(force_fill_submaps=True, submap_max_size=12, submap_overlap=5,
                                                                    submap_descriptor='mean_semantic'))
    assert (p.max_size, p.overlap, p.submap_descriptor, p.frame_descriptor_dist) == (12, 5, 'mean_semantic', None)
    with pytest.raises(ValueError):
        FillSubmapParams.from_submap_align_params(SubmapAlignParams(force_fill_submaps=False))
    with pytest.raises(ValueError):                                          # the radius mode's parameters still refuse this mode
        SubmapParams.from_submap_align_params(SubmapAlignParams(force_fill_submaps=True))


def test_borderline_detector_flags_what_it_should():
    a = np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]]); b = np.array([[3.0, 0.0, 0.0, 4.0, 1.0, 1.0]])
    assert not fo.borderline(a, b) and not fo.aabb_nearby(a, b)[0, 0]
    touch = b.copy(); touch[0, 0] = 1.0
    assert fo.aabb_nearby(a, touch)[0, 0] and fo.borderline(a, touch)        # touching boxes intersect, and are a borderline case
    off = b.copy(); off[0, 0] = 1.0 + 5e-10
    assert not fo.aabb_nearby(a, off)[0, 0] and fo.borderline(a, off)
    empty = np.array([[np.inf] * 3 + [-np.inf] * 3])
    assert not fo.aabb_nearby(a, empty)[0, 0] and not fo.aabb_nearby(empty, empty)[0, 0] and not fo.borderline(empty, empty) and not fo.borderline(a, empty)
    t = np.array([0.0, 8.0, 16.0])
    assert fo.borderline(slice_mean=[4.0 + 4e-10], traj_times=t) and not fo.borderline(slice_mean=[5.0, 15.0], traj_times=t)


# ---------------------------------------------------------------------------------------------
# submap_align_pools in AABB mode over a stand-in context
# ---------------------------------------------------------------------------------------------
class AabbStubContext(gg.PoolsStubContext):
    """tests/test_grid_gate_cpu.PoolsStubContext plus the two calls the AABB mode adds, through tests/_fill_boxes_oracle.py."""

    def __init__(self, n_objects, dim=3):
        super().__init__(n_objects, dim)
        self.boxes, self.aabb_gates, self.box_of = 0, 0, {}

    def submap_boxes_dev(self, S, F, cap, pool_ptr, count_ptr, T_ptr, box_ptr):
        self.boxes += 1; self.order.append("boxes")
        box = fo.boxes_oracle(_view(pool_ptr, (S * cap, F), np.float64), cap, _view(count_ptr, (S,), np.int32), _view(T_ptr, (S, 4, 4), np.float64))
        _view(box_ptr, (S, 6), np.float64)[:] = box
        self.box_of[int(box_ptr)] = box

    def grid_gate_aabb_dev(self, gp, S0, S1, pos0, T_w0, pos1, T_w1, dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, n_todo,
                           box0_ptr=None, box1_ptr=None, sim_in_ptr=None, time0_ptr=None, time1_ptr=None, desc0_ptr=None, desc1_ptr=None,
                           pos_gt0_ptr=None, pos_gt1_ptr=None):
        self.aabb_gates += 1; self.order.append("gate")
        assert sim_in_ptr is None and not any((gp.reserved0, gp.reserved1, gp.reserved[0], gp.reserved[1]))
        d = int(gp.desc_dim)
        side = lambda S, pos, gt, T, tm, desc: dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(gt, (S, 3), np.float64) if gt else None,
                                                    T_w=_view(T, (S, 4, 4), np.float64), time=_view(tm, (S,), np.float64),
                                                    desc=_view(desc, (S, d), np.float64) if d else None)
        o = fo.aabb_gate_oracle(side(S0, pos0, pos_gt0_ptr, T_w0, time0_ptr, desc0_ptr), side(S1, pos1, pos_gt1_ptr, T_w1, time1_ptr, desc1_ptr),
                                _view(box0_ptr, (S0, 6), np.float64), _view(box1_ptr, (S1, 6), np.float64),
                                gp.skip_distance, gp.desc_thresh, bool(gp.single_robot_lc), gp.lc_time_thresh)
        B = S0 * S1
        _view(dist, (S0, S1), np.float64)[:] = o["dist"]; _view(flags, (S0, S1), np.int32)[:] = o["flags"]
        _view(yaw, (S0, S1), np.float64)[:] = o["yaw_deg"]; _view(sim, (S0, S1), np.float64)[:] = o["sim"]
        _view(T_ij, (S0, S1, 4, 4), np.float64)[:] = o["T_ij"]
        n = o["n_todo"]
        _view(pairs, (B, 2), np.int32)[:n] = o["pairs"]; _view(T_ref, (B, 4, 4), np.float64)[:n] = o["T_ref"]
        _view(enable, (B,), np.int32)[:n] = o["enable"]; _view(n_todo, (1,), np.int32)[0] = n


def _fill_pools(descriptor=None, fill=True, context=AabbStubContext):
    """Two robots' maps of the same place (the same seed: pairs that align), each cut into pools on a stand-in."""
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    pools, segs = [], []
    for r in range(2):
        sg, traj, times = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
        if r == 1:
            for q in sg:
                q.id = int(q.id) + 100000
        table = MapTable.from_segments(reg, sg)
        if fill:
            fp = FillSubmapParams(12, 6, descriptor)
            centers, slices = fill_centers(table, traj, times, fp)
            pools.append(build_submap_pool(reg, table, centers, fp, ctx=fo.OracleFillContext(), device="cpu", fill=slices))
        else:
            sp = SubmapParams(max_size=12, radius=15.0, pruning_method='distance', submap_descriptor=descriptor)
            pools.append(build_submap_pool(reg, table, submap_centers(traj, times, sp), sp, ctx=so.OracleSubmapContext(), device="cpu"))
        segs.append(sg)
    reg.set_context(context(int(pools[0].pool.shape[0] + pools[1].pool.shape[0]), 3))
    return reg, pools, segs


@pytest.mark.parametrize("kind", ["force-fill", "force-fill-descriptor", "no-radius", "no-radius-gt"])
def test_pools_path_equals_grid_path_in_aabb_mode(kind):
    fill = kind.startswith("force-fill")
    descriptor = 'mean_semantic' if kind == "force-fill-descriptor" else None
    reg, pools, segs = _fill_pools(descriptor, fill)
    p = SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=fill, submap_radius=15.0 if fill else None, submap_max_size=12, submap_overlap=6,
                          submap_descriptor=descriptor, submap_descriptor_thresh=0.8)
    gt_poses, gt_of = (None, None), lambda r, s: None
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    if kind == "no-radius-gt":                                               # side 1 has ground truth (a shifted, turned copy): its box and T_w read it
        G = np.array([sa.transform_rm_roll_pitch(T.copy()) for T in pools[1].centers.pose_flu]) @ _lc_tail_shift()
        gt_poses, gt_of = (None, G), lambda r, s: G[s].copy() if r == 1 else None
        io = sa.SubmapAlignIO(lc_association_thresh=4, gt_available=(False, True))
    ctx = reg._context()
    got = sa.submap_align_pools(p, pools, io, registration=reg, gt_poses=gt_poses)
    assert ctx.boxes == 2 and ctx.aabb_gates == 1 and ctx.gates == 0 and ctx.tails == 1
    assert ctx.order[:3] == ["boxes", "boxes", "gate"] and ctx.order[-1] == "tail" and "batch" in ctx.order
    subs = [q.to_submaps(s) for q, s in zip(pools, segs)]
    for r in range(2):
        for sm in subs[r]:
            sm.pose_flu_gt = gt_of(r, sm.id)
    want = sa.submap_align_grid(p, subs, io, registration=reg, compute=_lc_tail.oracle_lc_compute)
    boxes = sorted(ctx.box_of.items())                                       # (allocation order is not asserted: either order gives the same flags)
    assert not fo.borderline(boxes[0][1], boxes[1][1]) and not fo.borderline(boxes[1][1], boxes[0][1])
    gg.assert_same_results(got, want)
    n, near = want.clipper_num_associations, ~np.isnan(want.robots_nearby_mat)
    assert (n >= 4).sum() >= 2, "no pair of the grid aligned: the comparison would show nothing"
    assert near.any() and (~near).any(), "every pair or no pair is nearby: the gate would show nothing"
    if descriptor:
        assert (want.similarity_mat < 0.8).any() and (want.similarity_mat >= 0.8).any()


def _lc_tail_shift():
    T = np.eye(4); c, s = np.cos(0.3), np.sin(0.3)
    T[:2, :2] = [[c, -s], [s, c]]; T[:3, 3] = [4.0, -3.0, 0.5]
    return T


def test_aabb_mode_is_refused_where_it_cannot_run():
    """A context without the new calls (the stand-in of tests/test_grid_gate_cpu.py) and pools of dim 2 keep the ValueError that
    names the other way."""
    reg, pools, _ = _fill_pools(None, True, context=gg.PoolsStubContext)
    p = SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=True)
    with pytest.raises(ValueError, match="to_submaps") as e:
        sa.submap_align_pools(p, pools, sa.SubmapAlignIO(), registration=reg)
    assert "submap_align_grid" in str(e.value) and reg._context().gates == 0
    reg2, pools2, _ = gg._pools("roman", None, dim=2)
    reg2.set_context(AabbStubContext(int(pools2[0].pool.shape[0] + pools2[1].pool.shape[0]), 2))
    with pytest.raises(ValueError, match="to_submaps") as e:
        sa.submap_align_pools(SubmapAlignParams(method="roman", semantics_dim=D, dim=2, submap_radius=None), pools2, sa.SubmapAlignIO(), registration=reg2)
    assert "no z" in str(e.value) and reg2._context().boxes == 0


# ---------------------------------------------------------------------------------------------
# the C-ABI boundary
# ---------------------------------------------------------------------------------------------
def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, nargs in ENTRY_POINTS.items():
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == nargs, s
    at = src.index("ROMAN_API int roman_submaps_fill_dev(")
    for ref in ("[REF roman/map/map.py:264-295]", "[REF roman/utils.py:160-169]", "[REF roman/map/map.py:133-139]"):
        assert ref in src[max(0, at - 4000):], ref
    assert "stay with the caller" not in src                                 # the sentence about the AABB mode is up to date


def test_struct_layout_matches_c(tmp_path):
    """The structs the new entries take are the existing ones: their mirrors still match what the C compiler lays out."""
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    'printf("gate %zu\\n", sizeof(roman_grid_gate_params_t));\nprintf("desc %zu\\n", sizeof(roman_submap_desc_t));\n'
                    'printf("T %zu\\n", offsetof(roman_submap_desc_t, T_center_odom));\nprintf("radius %zu\\n", offsetof(roman_grid_gate_params_t, radius));\n'
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    from roman_amd.runtime import submap_desc_dtype
    assert int(out["gate"]) == C.sizeof(_abi.RomanGridGateParams) and int(out["radius"]) == _abi.RomanGridGateParams.radius.offset
    assert int(out["desc"]) == C.sizeof(_abi.RomanSubmapDesc) == submap_desc_dtype().itemsize
    assert int(out["T"]) == _abi.RomanSubmapDesc.T_center_odom.offset == submap_desc_dtype().fields["T_center_odom"][1]


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    from roman_amd.runtime import grid_gate_params
    P = grid_gate_params(None)
    n = np.zeros(64, np.int64)
    v = C.c_void_p(n.ctypes.data)
    for fn in (lib.roman_grid_gate_aabb_dev, lib.roman_grid_gate_aabb):
        assert fn(None, C.byref(P), 0, 0, *([None] * 10), *([v] * 9), v, v, None) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
    for fn in (lib.roman_submap_boxes_dev, lib.roman_submap_boxes):
        assert fn(None, 1, 3, 4, v, v, v, v) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
    for fn in (lib.roman_submaps_fill_dev, lib.roman_submaps_fill):
        assert fn(None, 3, 4, 1, 3, v, None, 1, v, v, v, v, None, 0, None) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
