"""RANSAC loop closures over device-resident pools — TEST INFRASTRUCTURE shared by tests/test_ransac_lc_cpu.py
(stand-in context) and tests/test_gpu_ransac_lc.py (the device).

`ransac_lc_double()` is the CPU double of roman_ransac_lc_batch[_dev]: tests/_ransac_oracle.py (steps 1-7) per problem on columns
0-2 of the rows, then the tail oracle of tests/_lc_tail.py.  It is exact only away from the thresholds, so it ASSERTS that the
oracle flags no borderline hypothesis and no tie for any problem it is given: a borderline case fails loudly.
`RansacLcStubContext` adds ransac_lc_batch_dev (and the host form) to the stand-in contexts of tests/test_self_pools_cpu.py and
tests/test_fill_boxes_cpu.py, written through raw addresses like their other calls."""
import numpy as np

import _lc_tail
import _ransac_oracle as ro
from _stub_context import _view
from roman_amd import _abi
from roman_amd.runtime import LcInputs, LoopClosureResult, ransac_record_dtype, stats_dtype
from test_fill_boxes_cpu import AabbStubContext
from test_self_pools_cpu import SelfPoolsStubContext

_SOLVED = {}                # (P bytes, Q bytes, parameters) -> the oracle's answer: every distinct problem is solved once per session


def params_tuple(rp):
    return (int(rp.max_iteration), int(rp.round), float(rp.edge_len), float(rp.max_dist), float(rp.confidence), int(rp.seed))


def solve(orc, rp, P, Q):
    """One problem -> dict(rows (k, 2) int32, T (4, 4) NaN when there is no pose, status, n_assoc, n_hyp, n_scored, best_hyp,
    best_count, best_sse).  Asserts that the oracle saw no borderline hypothesis and no tie."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3); Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    if len(P) == 0 or len(Q) == 0:
        return dict(rows=np.zeros((0, 2), np.int32), T=np.full((4, 4), np.nan), status=_abi.ROMAN_ST_EMPTY_MAP, n_assoc=0, n_hyp=0, n_scored=0,
                    best_hyp=-1, best_count=0, best_sse=0.0)
    key = (P.tobytes(), Q.tobytes(), len(P), params_tuple(rp))
    if key not in _SOLVED:
        mi, rnd, el, md, cf, seed = params_tuple(rp)
        rows, T, res = ro.result(orc, P, Q, max_iteration=mi, round=rnd, edge_len=el, max_dist=md, confidence=cf, seed=seed)
        assert res.n_border == 0 and len(res.best_set) <= 1, "a borderline hypothesis or a tie: the double is exact only away from the thresholds"
        ok = T is not None
        if not res.best_set:                                 # nothing survived the prune: the record of the no-survivor exit
            out = dict(rows=rows, T=np.full((4, 4), np.nan), status=_abi.ROMAN_ST_INSUFFICIENT, n_assoc=0, n_hyp=res.n_hyp, n_scored=0, best_hyp=-1,
                       best_count=0, best_sse=0.0)
        else:
            h = res.best_set[0]
            out = dict(rows=rows, T=T if ok else np.full((4, 4), np.nan), status=_abi.ROMAN_ST_OK if ok else _abi.ROMAN_ST_INSUFFICIENT, n_assoc=len(rows),
                       n_hyp=res.n_hyp, n_scored=res.n_scored, best_hyp=h, best_count=res.best_count, best_sse=float(res.sse[h]))
        _SOLVED[key] = out
    return _SOLVED[key]


def ransac_double(orc, rp, rows, off1, n1, off2, n2, kmax):
    """roman_ransac_lc_batch's RANSAC half -> (assoc list, T (B, 4, 4), n_assoc (B,), status (B,), records (B,) ransac_record_dtype)."""
    rows = np.asarray(rows, dtype=np.float64)
    B = len(n1)
    assoc, T = [], np.full((B, 4, 4), np.nan)
    n = np.zeros(B, np.int32); status = np.zeros(B, np.int32); rec = np.zeros(B, dtype=ransac_record_dtype())
    for b in range(B):
        r = solve(orc, rp, rows[off1[b]:off1[b] + n1[b], :3], rows[off2[b]:off2[b] + n2[b], :3])
        st = r["status"] | (_abi.ROMAN_ST_ASSOC_TRUNCATED if r["n_assoc"] > kmax else 0)
        assoc.append(r["rows"][:kmax].copy()); T[b] = r["T"]; n[b] = r["n_assoc"]; status[b] = st
        rec[b] = (r["n_assoc"], st, r["n_hyp"], r["n_scored"], r["best_hyp"], r["best_count"], r["best_sse"], r["T"].reshape(16))
    return assoc, T, n, status, rec


def ransac_lc_double(orc, rp, rows, off1, n1, off2, n2, lc, kmax=None):
    """The CPU double of Context.ransac_lc_batch -> runtime.LoopClosureResult (stats zeros, ransac_records set)."""
    B = len(n1)
    if kmax is None:
        kmax = int(max(1, np.max(np.asarray(n1, np.int64) * np.asarray(n2)))) if B else 1
    assoc, T, n, status, rec = ransac_double(orc, rp, rows, off1, n1, off2, n2, kmax)
    records, acc = _lc_tail.lc_tail(lc, T, n, status)
    return LoopClosureResult(assoc, T, status, np.zeros(B, dtype=stats_dtype()), records, acc, ransac_records=rec)


class RansacLcStubContext(SelfPoolsStubContext, AabbStubContext):
    """The stand-ins of tests/test_self_pools_cpu.py (shared-segment removal) and tests/test_fill_boxes_cpu.py (boxes, AABB gate)
    in one context, plus roman_ransac_lc_batch_dev through the double above."""

    def __init__(self):
        super().__init__(3)
        self.ransacs = []                                    # (problems, row width, tail?) of every call

    def ransac_lc_batch_dev(self, rp, rows_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, rec_out_ptr, T_out_ptr=None, n_assoc_out_ptr=None,
                            status_out_ptr=None, lc_params=None, records_ptr=None, accepted_idx_ptr=None, n_accepted_ptr=None, counts_out_ptr=None,
                            **tail_ptrs):
        B = len(n1)
        self.ransacs.append((B, int(F), lc_params is not None)); self.order.append("ransac")
        assert F >= 3 and counts_out_ptr is None
        n_rows = int(max(np.max(np.asarray(off1) + n1), np.max(np.asarray(off2) + n2))) if B else 0
        assoc, T, n, status, rec = ransac_double(self.orc, rp, _view(rows_ptr, (n_rows, int(F)), np.float64), off1, n1, off2, n2, kmax)
        a_out = _view(assoc_out_ptr, (B, kmax, 2), np.int32)
        for b in range(B):
            a_out[b, :len(assoc[b])] = assoc[b]
        _view(rec_out_ptr, (B,), ransac_record_dtype())[:] = rec
        if T_out_ptr:
            _view(T_out_ptr, (B, 4, 4), np.float64)[:] = T
        if n_assoc_out_ptr:
            _view(n_assoc_out_ptr, (B,), np.int32)[:] = n
        if status_out_ptr:
            _view(status_out_ptr, (B,), np.int32)[:] = status
        if lc_params is not None:
            assert T_out_ptr and n_assoc_out_ptr and status_out_ptr
            self.lc_tail_dev(lc_params, B, T_out_ptr, n_assoc_out_ptr, status_out_ptr, records_ptr, accepted_idx_ptr, n_accepted_ptr, **tail_ptrs)

    def ransac_lc_batch(self, rp, rows, off1, n1, off2, n2, lc, kmax=None, counts=None):
        self.ransacs.append((len(n1), int(np.asarray(rows).shape[1]), True)); self.order.append("ransac-host")
        return ransac_lc_double(self.orc, rp, rows, off1, n1, off2, n2, lc, kmax)


def assert_same_matrices(got, want):
    """The result matrices of the pools path against the pair loop, with the tolerances of
    tests/test_grid_gate_cpu.assert_same_results — except that robots_nearby_mat is compared like the other float matrices (NaN
    pattern exact, values to 1e-12 relative): the pair loop takes one norm per pair, the gate one over the grid, and their
    summation orders differ by an ulp or two (tests/test_submap_align_grid_cpu.py allows the same between those two forms)."""
    from test_grid_gate_cpu import close
    assert np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
    for name in ("robots_nearby_mat", "T_ij_mat", "T_ij_hat_mat", "submap_yaw_diff_mat"):
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


def assert_same_edges(got, want, submaps, atol=1e-9):
    """The device's loop-closure edges of `got` against loop_closure_edges() of the pair-loop result `want`: the same pairs in
    the same order, the same transforms."""
    from roman_amd.align import submap_align as sa
    edges = sa.loop_closure_edges(want, submaps)
    assert np.array_equal(np.asarray(got.lc_edges["pairs"]).reshape(-1, 2), np.array([(i, j) for i, j, _ in edges], dtype=np.int64).reshape(-1, 2))
    for k, (_, _, T) in enumerate(edges):
        t, q = sa.transform_to_xyz_quat(T)
        np.testing.assert_allclose(got.lc_edges["t"][k], t, rtol=0, atol=atol)
        np.testing.assert_allclose(got.lc_edges["q"][k], q, rtol=0, atol=atol)
