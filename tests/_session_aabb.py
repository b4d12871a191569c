"""The bounding-box gate and the RANSAC baseline of a whole session — TEST INFRASTRUCTURE shared by the session
AABB tests.

`session_boxes_oracle()` and `session_gate_aabb_oracle()` are tests/_fill_boxes_oracle.py applied per submap and per block.
`SessionAabbStubContext` adds roman_session_boxes_dev and roman_session_gate_aabb_dev (and keeps roman_session_gate_dev and
roman_ransac_lc_batch_dev) on the stand-in contexts, written through raw addresses of host memory, so that submap_align_session
runs in AABB mode and with a RansacReg without a GPU.  `exact()` compares two results of one block bit for bit."""
import numpy as np

import _fill_boxes_oracle as fo
import _ransac_lc as rl
import _session as ss
import _session_stacked as sst
from _stub_context import _view
from test_fill_boxes_cpu import AabbStubContext


def session_boxes_oracle(pool, row0, count, T_odom_center):
    """pool (rows, F), submap g = rows [row0[g], row0[g] + count[g]) -> (S, 6), boxes_oracle per submap."""
    pool = np.asarray(pool, np.float64)
    T = np.asarray(T_odom_center, np.float64).reshape(-1, 4, 4)
    box = np.empty((len(count), 6))
    for g in range(len(count)):
        n, lo = int(count[g]), int(row0[g])
        box[g] = fo.boxes_oracle(pool[lo:lo + n], max(n, 1), [n], T[g:g + 1])[0]
    return box


def session_gate_aabb_oracle(arr, box, sub_off, blocks, has_gt, skip_distance=np.inf, desc_thresh=0.0, lc_time_thresh=0.0, sim_in=None, pair_off=None):
    """tests/_session.session_gate_oracle with aabb_gate_oracle per block; sim_in (pair_off[nb],): the similarity is given."""
    per, todo_off = [], [0]
    for b, (r0, r1, lc, _) in enumerate(np.asarray(blocks).reshape(-1, 4).tolist()):
        gt = arr.get("pos_gt") is not None and bool(has_gt[r0]) and bool(has_gt[r1])
        n0, n1 = int(sub_off[r0 + 1] - sub_off[r0]), int(sub_off[r1 + 1] - sub_off[r1])
        if n0 == 0 or n1 == 0:
            z = lambda *t: np.zeros((0,) + t)
            o = dict(dist=z(), flags=z(), yaw_deg=z(), sim=z(), T_ij=z(4, 4), pairs=np.zeros((0, 2), np.int32), T_ref=z(4, 4), enable=z(), n_todo=0)
        else:
            s_in = None if sim_in is None else np.asarray(sim_in)[int(pair_off[b]):int(pair_off[b + 1])].reshape(n0, n1)
            o = fo.aabb_gate_oracle(ss.side_of(arr, sub_off, r0, gt), ss.side_of(arr, sub_off, r1, gt), box[sub_off[r0]:sub_off[r0 + 1]],
                                    box[sub_off[r1]:sub_off[r1 + 1]], skip_distance, desc_thresh, bool(lc), lc_time_thresh, sim_in=s_in)
        o["gpairs"] = o["pairs"].astype(np.int64) + np.array([sub_off[r0], sub_off[r1]], dtype=np.int64)
        per.append(o); todo_off.append(todo_off[-1] + o["n_todo"])
    cat = lambda k, tail: np.concatenate([o[k].reshape((-1,) + tail) for o in per]) if per else np.zeros((0,) + tail)
    return dict(dist=cat("dist", ()), flags=cat("flags", ()).astype(np.int32), yaw_deg=cat("yaw_deg", ()), sim=cat("sim", ()), T_ij=cat("T_ij", (4, 4)),
                pairs=cat("gpairs", (2,)).astype(np.int32), T_ref=cat("T_ref", (4, 4)), enable=cat("enable", ()).astype(np.int32),
                todo_off=np.array(todo_off, dtype=np.int32), per=per)


class SessionAabbStubContext(rl.RansacLcStubContext):
    """The stand-in with every call of the pools path (radius and AABB gate, shared-segment removal, RANSAC) plus the session's:
    roman_session_gate_dev as tests/_session.SessionStubContext has it, roman_session_boxes_dev and roman_session_gate_aabb_dev."""
    session_gate_dev = ss.SessionStubContext.session_gate_dev

    def __init__(self):
        super().__init__()
        self.session_gates, self.session_aabb_gates, self.session_boxes = 0, 0, []      # session_boxes: (row0, count, T, box) of every call

    def session_boxes_dev(self, S, F, pool_ptr, row0_ptr, count_ptr, T_ptr, box_ptr):
        self.order.append("session_boxes")
        row0, count = _view(row0_ptr, (S,), np.int64).copy(), _view(count_ptr, (S,), np.int32).copy()
        T = _view(T_ptr, (S, 4, 4), np.float64).copy()
        box = session_boxes_oracle(_view(pool_ptr, (int((row0 + count).max()), F), np.float64), row0, count, T)
        _view(box_ptr, (S, 6), np.float64)[:] = box
        self.session_boxes.append((row0, count, T, box))

    def session_gate_aabb_dev(self, gp, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos, T_w,
                              dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, box_ptr, time_ptr=None, desc_ptr=None, pos_gt_ptr=None,
                              has_gt_ptr=None, sim_in_ptr=None):
        self.session_aabb_gates += 1; self.order.append("session_gate")
        self.table_robots = len(sub_off) - 1
        R, nb, S, d = len(sub_off) - 1, len(blocks), int(sub_off[-1]), int(gp.desc_dim)
        want = ss.tables(np.diff(sub_off).tolist(), [tuple(b[:3]) for b in np.asarray(blocks).tolist()])
        for host, dev_ptr, w in zip((sub_off, blocks, pair_off, tile_off), (sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr), want):
            assert np.array_equal(host, w) and host.dtype == w.dtype
            assert np.array_equal(_view(dev_ptr, w.shape, w.dtype), w), "the device copy of a table differs from the host copy"
        assert not gp.single_robot_lc and not any((gp.reserved0, gp.reserved1, gp.reserved[0], gp.reserved[1]))
        assert sim_in_ptr is None or d == 0
        arr = dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(pos_gt_ptr, (S, 3), np.float64) if pos_gt_ptr else None,
                   T_w=_view(T_w, (S, 4, 4), np.float64), time=_view(time_ptr, (S,), np.float64) if time_ptr else None,
                   desc=_view(desc_ptr, (S, d), np.float64) if d else None)
        has_gt = _view(has_gt_ptr, (R,), np.int32) if has_gt_ptr else np.zeros(R, np.int32)
        total = int(pair_off[-1])
        o = session_gate_aabb_oracle(arr, _view(box_ptr, (S, 6), np.float64), sub_off, blocks, has_gt, gp.skip_distance, gp.desc_thresh, gp.lc_time_thresh,
                                     sim_in=_view(sim_in_ptr, (total,), np.float64) if sim_in_ptr else None, pair_off=pair_off)
        n = int(o["todo_off"][-1])
        _view(dist, (total,), np.float64)[:] = o["dist"]; _view(flags, (total,), np.int32)[:] = o["flags"]
        _view(yaw, (total,), np.float64)[:] = o["yaw_deg"]
        if not sim_in_ptr:
            _view(sim, (total,), np.float64)[:] = o["sim"]
        _view(T_ij, (total, 4, 4), np.float64)[:] = o["T_ij"]
        _view(pairs, (total, 2), np.int32)[:n] = o["pairs"]; _view(T_ref, (total, 4, 4), np.float64)[:n] = o["T_ref"]
        _view(enable, (total,), np.int32)[:n] = o["enable"]; _view(todo_off, (nb + 1,), np.int32)[:] = o["todo_off"]


class SessionAabbStackedStubContext(sst.SessionStackedStubContext):
    """The stand-in of tests/_session_stacked.py (frame selection, the stacked similarity per grid and per session) with the
    bounding-box calls: the session's two from SessionAabbStubContext, roman_submap_boxes_dev from tests/test_fill_boxes_cpu.py, and
    roman_grid_gate_aabb_dev WITH a given similarity (that file's stand-in takes none)."""
    submap_boxes_dev = AabbStubContext.submap_boxes_dev
    session_boxes_dev = SessionAabbStubContext.session_boxes_dev
    session_gate_aabb_dev = SessionAabbStubContext.session_gate_aabb_dev

    def __init__(self):
        super().__init__()
        self.boxes, self.aabb_gates, self.box_of, self.session_aabb_gates, self.session_boxes = 0, 0, {}, 0, []

    def grid_gate_aabb_dev(self, gp, S0, S1, pos0, T_w0, pos1, T_w1, dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, n_todo,
                           box0_ptr=None, box1_ptr=None, sim_in_ptr=None, time0_ptr=None, time1_ptr=None, desc0_ptr=None, desc1_ptr=None,
                           pos_gt0_ptr=None, pos_gt1_ptr=None):
        self.aabb_gates += 1; self.order.append("gate")
        d = int(gp.desc_dim)
        assert (sim_in_ptr is None or d == 0) and not any((gp.reserved0, gp.reserved1, gp.reserved[0], gp.reserved[1]))
        side = lambda S, pos, gt, T, tm, desc: dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(gt, (S, 3), np.float64) if gt else None,
                                                    T_w=_view(T, (S, 4, 4), np.float64), time=_view(tm, (S,), np.float64),
                                                    desc=_view(desc, (S, d), np.float64) if d else None)
        o = fo.aabb_gate_oracle(side(S0, pos0, pos_gt0_ptr, T_w0, time0_ptr, desc0_ptr), side(S1, pos1, pos_gt1_ptr, T_w1, time1_ptr, desc1_ptr),
                                _view(box0_ptr, (S0, 6), np.float64), _view(box1_ptr, (S1, 6), np.float64), gp.skip_distance, gp.desc_thresh,
                                bool(gp.single_robot_lc), gp.lc_time_thresh, sim_in=_view(sim_in_ptr, (S0, S1), np.float64).copy() if sim_in_ptr else None)
        B, n = S0 * S1, o["n_todo"]
        _view(dist, (S0, S1), np.float64)[:] = o["dist"]; _view(flags, (S0, S1), np.int32)[:] = o["flags"]
        _view(yaw, (S0, S1), np.float64)[:] = o["yaw_deg"]; _view(T_ij, (S0, S1, 4, 4), np.float64)[:] = o["T_ij"]
        if not sim_in_ptr:
            _view(sim, (S0, S1), np.float64)[:] = o["sim"]
        _view(pairs, (B, 2), np.int32)[:n] = o["pairs"]; _view(T_ref, (B, 4, 4), np.float64)[:n] = o["T_ref"]
        _view(enable, (B,), np.int32)[:n] = o["enable"]; _view(n_todo, (1,), np.int32)[0] = n


MATRICES = ("robots_nearby_mat", "clipper_num_associations", "T_ij_mat", "T_ij_hat_mat", "submap_yaw_diff_mat", "clipper_angle_mat", "clipper_dist_mat")


def exact(got, want, stand_in_sim_terms=0):
    """Two results of one block, bit for bit: every matrix (NaN where NaN), every association list, the similarity, the edges.
    stand_in_sim_terms = d, for runs over the NumPy stand-in only: its similarity is a BLAS product (tests/_grid_gate_oracle.py)
    whose summation order depends on where the arrays lie in memory, so the same d-term dot product of two unit-scale vectors may
    come out in two orders, at most d ulp of 1 apart (d * 2^-52); which pairs it gates is still compared exactly, through every
    other matrix.  The device's similarity has a fixed order and is compared bit for bit (0)."""
    for name in MATRICES:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name
    n0, n1 = want.clipper_num_associations.shape
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert (got.similarity_mat is None) == (want.similarity_mat is None)
    if want.similarity_mat is not None:
        if stand_in_sim_terms:
            np.testing.assert_allclose(got.similarity_mat, want.similarity_mat, rtol=0, atol=stand_in_sim_terms * 2.0 ** -52, equal_nan=True)
        else:
            assert np.array_equal(got.similarity_mat, want.similarity_mat, equal_nan=True)
    assert (got.lc_edges is None) == (want.lc_edges is None)
    if want.lc_edges is not None:
        for k in ("pairs", "t", "q"):
            assert np.array_equal(got.lc_edges[k], want.lc_edges[k]), k
    assert len(got.timing_list) == len(want.timing_list)
