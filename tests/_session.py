"""A whole session in one call — TEST INFRASTRUCTURE shared by the session tests.

`session_gate_oracle()` is the expectation for roman_session_gate*: pass 1 of tests/_grid_gate_oracle.py applied per block and
concatenated, the compact list as global submap indices.  `SessionStubContext` adds the call to the stand-in contexts (the gate
written through raw addresses of host memory), so that submap_align_session runs without a GPU.  `compare()` holds the
tolerances of tests/test_gpu_submap_align_pools.py between two results of one block."""
import numpy as np

import _grid_gate_oracle as go
from _stub_context import _view
from test_self_pools_cpu import SelfPoolsStubContext


def robot_view(segs, traj, times, r, keep=1.0, first_pose=0, last_pose=None, id_step=100000, d=16):
    """Robot r's own map of a place: a random `keep` fraction of the segments, every centre a few cm off, the descriptor slightly
    off, ids of its own, and the poses [first_pose, last_pose) of the drive — so that no two robots of a session have the same
    pool rows, the same number of submaps or the same number of segments (true matches across robots remain).
    -> (segments, trajectory, times)."""
    import copy
    rng = np.random.default_rng(9000 + r)
    pick = np.sort(rng.permutation(len(segs))[:max(1, int(round(keep * len(segs))))])
    out = []
    for k in pick.tolist():
        q = copy.deepcopy(segs[k])
        q.id = int(segs[k].id) + id_step * r
        q.centroid = np.asarray(q.centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(q.centroid))
        if getattr(q, "semantic_descriptor", None) is not None:
            v = np.asarray(q.semantic_descriptor, dtype=np.float64) + 0.02 * rng.standard_normal(d) / np.sqrt(d)
            q.semantic_descriptor = v / np.linalg.norm(v)
        out.append(q)
    sl = slice(first_pose, last_pose)
    return out, [np.array(T) for T in traj[sl]], np.asarray(times)[sl].copy()


def tables(counts, blocks):
    """-> sub_off, blocks (nb, 4), pair_off, tile_off, written out independently of runtime.session_tables."""
    sub_off = np.zeros(len(counts) + 1, dtype=np.int32)
    for r, n in enumerate(counts):
        sub_off[r + 1] = sub_off[r] + n
    blk = np.zeros((len(blocks), 4), dtype=np.int32)
    pair_off, tile_off = np.zeros(len(blocks) + 1, dtype=np.int64), np.zeros(len(blocks) + 1, dtype=np.int64)
    for b, (r0, r1, lc) in enumerate(blocks):
        blk[b] = (r0, r1, int(lc), 0)
        pair_off[b + 1] = pair_off[b] + counts[r0] * counts[r1]
        tile_off[b + 1] = tile_off[b] + counts[r0] * ((counts[r1] + 3) // 4)
    return sub_off, blk, pair_off, tile_off


def side_of(arr, sub_off, r, use_gt):
    """Robot r's rows of the session-wide arrays as a side of tests/_grid_gate_oracle.py."""
    lo, hi = int(sub_off[r]), int(sub_off[r + 1])
    return dict(pos=arr["pos"][lo:hi], pos_gt=arr["pos_gt"][lo:hi] if use_gt else None, T_w=arr["T_w"][lo:hi].reshape(-1, 4, 4),
                time=None if arr.get("time") is None else arr["time"][lo:hi], desc=None if arr.get("desc") is None else arr["desc"][lo:hi])


def session_gate_oracle(arr, sub_off, blocks, has_gt, radius, skip_distance=np.inf, desc_thresh=0.0, lc_time_thresh=0.0):
    """arr: dict(pos (S, 3), pos_gt (S, 3) or None, T_w (S, 4, 4), time (S,), desc (S, d) or None) -> the dense outputs
    concatenated block by block, the compact outputs with global indices, todo_off, and the per-block oracle results."""
    per, todo_off = [], [0]
    for r0, r1, lc, _ in np.asarray(blocks).reshape(-1, 4).tolist():
        gt = arr.get("pos_gt") is not None and bool(has_gt[r0]) and bool(has_gt[r1])
        if sub_off[r0 + 1] == sub_off[r0] or sub_off[r1 + 1] == sub_off[r1]:       # an empty block: nothing dense, nothing compact
            z = lambda *t: np.zeros((0,) + t)
            o = dict(dist=z(), flags=z(), yaw_deg=z(), sim=z(), T_ij=z(4, 4), pairs=np.zeros((0, 2), np.int32), T_ref=z(4, 4), enable=z(), n_todo=0)
        else:
            o = go.grid_gate_oracle(side_of(arr, sub_off, r0, gt), side_of(arr, sub_off, r1, gt), radius, skip_distance, desc_thresh, bool(lc), lc_time_thresh)
        o["gpairs"] = o["pairs"].astype(np.int64) + np.array([sub_off[r0], sub_off[r1]], dtype=np.int64)
        per.append(o); todo_off.append(todo_off[-1] + o["n_todo"])
    cat = lambda k, tail: np.concatenate([o[k].reshape((-1,) + tail) for o in per]) if per else np.zeros((0,) + tail)
    return dict(dist=cat("dist", ()), flags=cat("flags", ()).astype(np.int32), yaw_deg=cat("yaw_deg", ()), sim=cat("sim", ()), T_ij=cat("T_ij", (4, 4)),
                pairs=cat("gpairs", (2,)).astype(np.int32), T_ref=cat("T_ref", (4, 4)), enable=cat("enable", ()).astype(np.int32),
                todo_off=np.array(todo_off, dtype=np.int32), per=per)


class SessionStubContext(SelfPoolsStubContext):
    """SelfPoolsStubContext plus roman_session_gate_dev through session_gate_oracle()."""

    def __init__(self, dim=3):
        super().__init__(dim)
        self.session_gates = 0

    def session_gate_dev(self, gp, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos, T_w,
                         dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, time_ptr=None, desc_ptr=None, pos_gt_ptr=None, has_gt_ptr=None):
        self.session_gates += 1; self.order.append("session_gate")
        self.table_robots = len(sub_off) - 1                 # entries of the robot table: more than robots where a robot has several views
        R, nb, S, d = len(sub_off) - 1, len(blocks), int(sub_off[-1]), int(gp.desc_dim)
        counts = np.diff(sub_off).tolist()
        want = tables(counts, [tuple(b[:3]) for b in np.asarray(blocks).tolist()])
        for host, dev_ptr, w in zip((sub_off, blocks, pair_off, tile_off), (sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr), want):
            assert np.array_equal(host, w) and host.dtype == w.dtype
            assert np.array_equal(_view(dev_ptr, w.shape, w.dtype), w), "the device copy of a table differs from the host copy"
        assert gp.radius >= 0 and not gp.single_robot_lc and not any((gp.reserved0, gp.reserved1, gp.reserved[0], gp.reserved[1]))
        arr = dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(pos_gt_ptr, (S, 3), np.float64) if pos_gt_ptr else None,
                   T_w=_view(T_w, (S, 4, 4), np.float64), time=_view(time_ptr, (S,), np.float64) if time_ptr else None,
                   desc=_view(desc_ptr, (S, d), np.float64) if d else None)
        has_gt = _view(has_gt_ptr, (R,), np.int32) if has_gt_ptr else np.zeros(R, np.int32)
        o = session_gate_oracle(arr, sub_off, blocks, has_gt, gp.radius, gp.skip_distance, gp.desc_thresh, gp.lc_time_thresh)
        total, n = int(pair_off[-1]), int(o["todo_off"][-1])
        _view(dist, (total,), np.float64)[:] = o["dist"]; _view(flags, (total,), np.int32)[:] = o["flags"]
        _view(yaw, (total,), np.float64)[:] = o["yaw_deg"]; _view(sim, (total,), np.float64)[:] = o["sim"]
        _view(T_ij, (total, 4, 4), np.float64)[:] = o["T_ij"]
        _view(pairs, (total, 2), np.int32)[:n] = o["pairs"]; _view(T_ref, (total, 4, 4), np.float64)[:n] = o["T_ref"]
        _view(enable, (total,), np.int32)[:n] = o["enable"]; _view(todo_off, (nb + 1,), np.int32)[:] = o["todo_off"]


def compare(got, want):
    """Two results of one block: exact where tests/test_gpu_submap_align_pools.py is exact, its bounds elsewhere (1e-12 for poses and
    edges, 1e-9 for the angle and distance matrices)."""
    n = want.clipper_num_associations
    assert got.clipper_num_associations.shape == n.shape
    assert np.array_equal(got.clipper_num_associations, n, equal_nan=True)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    for i in range(n.shape[0]):
        for j in range(n.shape[1]):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    for name in ("T_ij_mat", "T_ij_hat_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
    for name in ("clipper_angle_mat", "clipper_dist_mat", "submap_yaw_diff_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    assert (got.similarity_mat is None) == (want.similarity_mat is None)
    if want.similarity_mat is not None:
        np.testing.assert_allclose(got.similarity_mat, want.similarity_mat, rtol=0, atol=1e-12, equal_nan=True)
    assert (got.lc_edges is None) == (want.lc_edges is None)
    if want.lc_edges is not None:
        assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
        np.testing.assert_allclose(got.lc_edges["t"], want.lc_edges["t"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got.lc_edges["q"], want.lc_edges["q"], rtol=0, atol=1e-12)
    assert len(got.timing_list) == len(want.timing_list)
