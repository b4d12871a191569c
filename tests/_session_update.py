"""A session that grows — TEST INFRASTRUCTURE shared by the session-update tests.

`SessionUpdateStubContext` adds roman_session_gate_list_dev to tests/_session.SessionStubContext: the whole-grid oracle of
tests/_session.py (tests/_grid_gate_oracle.py per block) read at the listed pairs, the compact list in list order.  It records
every list it is handed.  With boxes or a given similarity the whole-grid oracle is the one of tests/_session_aabb.py or of
tests/_session_stacked.py (`SessionUpdateAabbStubContext`, `SessionUpdateStackedStubContext`).  `pool_prefix()` cuts a pool
back to its first k submaps — a session at an earlier step —, `equal()` compares two results of one block entry by entry
(everything but timing_list)."""
import dataclasses

import numpy as np

import _grid_gate_oracle as go
import _session as ss
import _session_aabb as sx
import _session_stacked as sst
from _stub_context import _view


class ListGateCalls:
    """roman_session_gate_list_dev for any stand-in context: mixed in IN FRONT of the context that serves the rest of the mode."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.lists, self.totals = [], []

    def session_gate_list_dev(self, gp, sub_off, blocks, pair_off, pair_list, sub_off_ptr, blocks_ptr, pair_off_ptr, list_ptr, pos, T_w,
                              dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, time_ptr=None, desc_ptr=None, pos_gt_ptr=None, has_gt_ptr=None,
                              sim_in_ptr=None, box_ptr=None):
        assert sim_in_ptr is None or gp.desc_dim == 0, "with a given similarity desc_dim must be 0"
        self.order.append("session_gate_list")
        R, nb, S, d, L = len(sub_off) - 1, len(blocks), int(sub_off[-1]), int(gp.desc_dim), len(pair_list)
        want = ss.tables(np.diff(sub_off).tolist(), [tuple(b[:3]) for b in np.asarray(blocks).tolist()])
        for host, dev_ptr, w in zip((sub_off, blocks, pair_off), (sub_off_ptr, blocks_ptr, pair_off_ptr), want):
            assert np.array_equal(host, w) and host.dtype == w.dtype
            assert np.array_equal(_view(dev_ptr, w.shape, w.dtype), w), "the device copy of a table differs from the host copy"
        lst = np.asarray(pair_list)
        assert lst.dtype == np.int32 and lst.shape == (L, 3) and np.array_equal(_view(list_ptr, (L, 3), np.int32), lst)
        keys = [tuple(x) for x in lst.tolist()]
        assert keys == sorted(set(keys)), "the list is not strictly ascending"
        self.lists.append(lst.copy()); self.totals.append(int(pair_off[-1]))
        arr = dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(pos_gt_ptr, (S, 3), np.float64) if pos_gt_ptr else None,
                   T_w=_view(T_w, (S, 4, 4), np.float64), time=_view(time_ptr, (S,), np.float64) if time_ptr else None,
                   desc=_view(desc_ptr, (S, d), np.float64) if d else None)
        has_gt = _view(has_gt_ptr, (R,), np.int32) if has_gt_ptr else np.zeros(R, np.int32)
        given = _view(sim_in_ptr, (int(pair_off[-1]),), np.float64).copy() if sim_in_ptr else None
        if box_ptr:                                          # the whole-grid oracle of tests/_session_aabb.py
            o = sx.session_gate_aabb_oracle(arr, _view(box_ptr, (S, 6), np.float64), sub_off, blocks, has_gt, gp.skip_distance, gp.desc_thresh,
                                            gp.lc_time_thresh, sim_in=given, pair_off=pair_off)
        elif given is not None:                              # tests/_session_stacked.py: the gate without descriptors, its classes from the similarity
            o = ss.session_gate_oracle(arr, sub_off, blocks, has_gt, gp.radius, gp.skip_distance, 0.0, gp.lc_time_thresh)
            o["flags"] = sst.gate_from_sim(o, given, sub_off, blocks, gp.desc_thresh, arr["time"] if time_ptr else np.zeros(S), gp.lc_time_thresh)["flags"]
        else:
            o = ss.session_gate_oracle(arr, sub_off, blocks, has_gt, gp.radius, gp.skip_distance, gp.desc_thresh, gp.lc_time_thresh)
        if given is not None:                                # (sim[l] is the pair's entry of sim_in)
            o["sim"] = given
        blk =np.asarray(blocks).reshape(-1, 4)
        b, i, j = (lst[:, k].astype(np.int64) for k in range(3))
        n1 = np.diff(sub_off)[blk[:, 1]].astype(np.int64)
        idx = pair_off[b] + i * n1[b] + j
        assert ((i < np.diff(sub_off)[blk[b, 0]]) & (j < n1[b])).all()
        fl = o["flags"][idx]
        todo = (fl & go.TODO) != 0
        gi, gj = sub_off[blk[b, 0]] + i, sub_off[blk[b, 1]] + j
        n = int(todo.sum())
        _view(dist, (L,), np.float64)[:] = o["dist"][idx]; _view(flags, (L,), np.int32)[:] = fl
        _view(yaw, (L,), np.float64)[:] = o["yaw_deg"][idx]; _view(sim, (L,), np.float64)[:] = o["sim"][idx]
        _view(T_ij, (L, 4, 4), np.float64)[:] = o["T_ij"][idx]
        _view(pairs, (L, 2), np.int32)[:n] = np.stack([gi, gj], axis=1)[todo]
        _view(T_ref, (L, 4, 4), np.float64)[:n] = o["T_ij"][idx][todo]
        en = np.ones(L, dtype=np.int32)
        if arr["time"] is not None:
            en[(blk[b, 2] != 0) & (np.abs(arr["time"][gi] - arr["time"][gj]) < gp.lc_time_thresh)] = 0
        _view(enable, (L,), np.int32)[:n] = en[todo]
        _view(todo_off, (nb + 1,), np.int32)[:] = np.concatenate([[0], np.cumsum(np.bincount(b[todo], minlength=nb))])


class SessionUpdateStubContext(ListGateCalls, ss.SessionStubContext):
    """The radius gate."""


class SessionUpdateAabbStubContext(ListGateCalls, sx.SessionAabbStubContext):
    """The bounding-box gate: roman_session_boxes_dev in front of the list gate, which reads the boxes."""


class SessionUpdateStackedStubContext(ListGateCalls, sst.SessionStackedStubContext):
    """Stacked frame descriptors: roman_session_stacked_sim_dev over whole blocks in front of the list gate, which reads it."""


def pool_prefix(pool, k, blank=()):
    """The first k submaps of `pool` as a pool of its own (rows, counts, ids, centres, descriptors, frame masks and counts — the
    frame table is the map's, one row per frame, and stays whole); `blank`: submaps that hold nothing yet (count 0)."""
    c = pool.centers
    cen = dataclasses.replace(c, **{f.name: getattr(c, f.name)[:k] for f in dataclasses.fields(c)})
    count = pool.count[:k].copy()
    count[np.array([s for s in blank if s < k], dtype=np.int64)] = 0
    cut = lambda a, n: None if a is None else a[:n]
    return dataclasses.replace(pool, pool=pool.pool[:k * pool.cap], count=count, src=pool.src[:k], ids=pool.ids[:k], status=pool.status[:k],
                               desc=cut(pool.desc, k), centers=cen, desc_dev=cut(pool.desc_dev, k), ids_dev=cut(pool.ids_dev, k * pool.cap),
                               frame_mask=cut(pool.frame_mask, k), frame_n=cut(pool.frame_n, k))


def equal(got, want, exact=True, sim_atol=0.0):
    """Two results of one block: every matrix, the associations, the edges and the hypotheses; only timing_list may differ.
    exact=False: the bounds of tests/_session.compare for what two runs of a solver may round differently.  sim_atol: the bound
    on similarity_mat alone — for the NumPy stand-in, whose matrix product rounds a pair's cosine differently in grids of
    different shapes (tests/_session.compare's 1e-12); the device adds every pair's products in one fixed order: 0."""
    same = (lambda a, b: np.array_equal(a, b, equal_nan=True)) if exact else \
        (lambda a, b: np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=0, atol=1e-9, equal_nan=True))
    for name in ("robots_nearby_mat", "clipper_angle_mat", "clipper_dist_mat", "clipper_num_associations", "similarity_mat", "submap_yaw_diff_mat",
                 "T_ij_mat", "T_ij_hat_mat"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), name
        if a is not None:
            if name == "similarity_mat" and sim_atol:
                assert a.shape == b.shape and np.allclose(a, b, rtol=0, atol=sim_atol, equal_nan=True), name
                continue
            assert a.shape == b.shape and same(a, b), name
    for name in ("clipper_num_associations", "robots_nearby_mat", "T_ij_mat"):
        assert np.array_equal(getattr(got, name), getattr(want, name), equal_nan=True), name
    n = want.clipper_num_associations.shape
    for i in range(n[0]):
        for j in range(n[1]):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert (got.lc_edges is None) == (want.lc_edges is None)
    if want.lc_edges is not None:
        assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
        assert same(got.lc_edges["t"], want.lc_edges["t"]) and same(got.lc_edges["q"], want.lc_edges["q"])
    assert (got.hypotheses is None) == (want.hypotheses is None)
    if want.hypotheses is not None:
        assert sorted(got.hypotheses) == sorted(want.hypotheses)
        for key, hw in want.hypotheses.items():
            for a, b in zip(got.hypotheses[key], hw):
                assert np.array_equal(a[0], b[0]) and a[3:5] == b[3:5] and same(a[2], b[2]) and (a[5] is None) == (b[5] is None), key
    assert got.submap_align_params.single_robot_lc == want.submap_align_params.single_robot_lc
    assert tuple(got.submap_io.gt_available) == tuple(want.submap_io.gt_available)
