"""RANSAC loop closures on the device-resident pools path without a GPU: submap_align_pools(method='ransac')
over the stand-in context of tests/_ransac_lc.py against the pair-loop form submap_align(compute=ro.compute_double(orc)) on
to_submaps() of the same pools — both sides go through tests/_ransac_oracle.py, which asserts that no hypothesis is borderline —,
the stride (a pool built for RomanRegistration serves the baseline as it is), the chunking rule, the refusals, the factory.

Tolerances are those of tests/test_grid_gate_cpu.assert_same_results, with one exception that is written down here: the pair loop
takes the norm of one difference vector per pair and the gate the norm over the whole grid, whose summation order differs, so
robots_nearby_mat agrees in its NaN pattern exactly and in its values to 1e-12 relative (a few ulp) — the same allowance
tests/test_submap_align_grid_cpu.py makes between the pair loop and the grid form."""
import dataclasses

import numpy as np
import pytest

import _ransac_lc as rl
import _ransac_oracle as ro
import _self_pools as sp
import _submaps_oracle as so
import test_grid_gate_cpu as gg
from roman_amd import _abi, synth
from roman_amd.align import RansacReg, SubmapAlignParams
from roman_amd.align import batch as ab
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
from roman_amd.runtime import LcInputs

D = 16
THRESH = 4
ITER, ROUND = 2048, 256


def _ransac_reg(ctx=None):
    reg = RansacReg(max_iteration=ITER, round=ROUND)
    if ctx is not None:
        reg.set_context(ctx)
    return reg


def _maps():
    """Two robots' maps of the same place (the same seed: pairs that align), the second with its own ids and, far from everything
    else, one more pose with two segments: a submap RANSAC cannot sample three distinct objects from."""
    out = []
    for r in range(2):
        sg, traj, times = synth.make_map(60, D, seed=31, n_poses=24, dt=8.0)
        traj, times = list(traj), np.asarray(times, dtype=np.float64)
        if r == 1:
            for q in sg:
                q.id = int(q.id) + 100000
            extra, _, _ = synth.make_map(2, D, seed=77, n_poses=2, dt=1.0)
            T = np.eye(4); T[:3, 3] = [200.0, 0.0, 0.0]
            for k, q in enumerate(extra):
                q.id = 900000 + k
                q.centroid = np.array([200.0 + 3.0 * k, 1.0 - 2.0 * k, 0.5]).reshape(np.shape(q.centroid))
                q.first_seen = q.last_seen = float(times[-1] + 8.0)
            sg = sg + extra; traj = traj + [T]; times = np.concatenate([times, [times[-1] + 8.0]])
        out.append((sg, traj, times))
    return out


def _build(method, descriptor=None, dists=(45.0, 35.0), ctx=None, device="cpu"):
    """-> (pools, segments), packed with `method`'s registration: 3-6 submaps of at most 8 objects per side.  On host tensors
    through the submap oracle, or (tests/test_gpu_ransac_lc.py) on `device` through the real context `ctx`."""
    reg = SubmapAlignParams(method=method, semantics_dim=D).get_object_registration()
    pools, segs = [], []
    for (sg, traj, times), dist in zip(_maps(), dists):
        params = SubmapParams(max_size=8, radius=15.0, distance=dist, time_threshold=np.inf, pruning_method='distance', submap_descriptor=descriptor)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=ctx or so.OracleSubmapContext(),
                                       device=device))
        segs.append(sg)
    return pools, segs


@pytest.fixture(scope="module")
def built():
    return {"ransac": _build("ransac"), "roman": _build("roman", 'mean_semantic')}


def _self_pool(ctx=None, device="cpu"):
    """One robot, two laps (tests/_self_pools.two_lap_map): submaps of a lap share segments, submaps of different laps hold true matches."""
    reg = _ransac_reg()
    segs, traj, times = sp.two_lap_map(n_lap=60)
    params = SubmapParams(max_size=8, radius=15.0, distance=25.0, time_threshold=sp.TIME_THRESH, pruning_method='time')
    pool = build_submap_pool(reg, MapTable.from_segments(reg, segs), submap_centers(traj, times, params), params, ctx=ctx or so.OracleSubmapContext(), device=device)
    return pool, segs


CONFIGS = ["radius-grid", "self-shared-ids", "aabb", "mean-semantic-over-roman-pool"]


def _config(kind, built, self_pool=None):
    base = dict(method="ransac", ransac_iter=ITER, submap_max_size=8)
    io = sa.SubmapAlignIO(lc_association_thresh=THRESH)
    if kind == "radius-grid":
        return SubmapAlignParams(**base, submap_radius=15.0), io, built["ransac"]
    if kind == "aabb":
        return SubmapAlignParams(**base, submap_radius=None), io, built["ransac"]
    if kind == "mean-semantic-over-roman-pool":
        return SubmapAlignParams(**base, semantics_dim=D, submap_radius=15.0, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.5), io, built["roman"]
    pool, segs = self_pool or _self_pool()
    p = SubmapAlignParams(**base, submap_radius=15.0, single_robot_lc=True, single_robot_lc_time_thresh=200.0)
    return p, io, ([pool, pool], [segs, segs])


def _pair_loop(orc, p, io, pools, segs):
    subs = [q.to_submaps(s) for q, s in zip(pools, segs)]
    return sa.submap_align(p, subs, io, registration=_ransac_reg(), compute=ro.compute_double(orc)), subs


def _registered(want, ctx):
    """Status of every problem the stand-in solved, in call order (the double caches by problem)."""
    return np.concatenate([np.atleast_1d(s) for s in ctx.statuses]) if ctx.statuses else np.zeros(0, np.int32)


class _Ctx(rl.RansacLcStubContext):
    """... that also remembers the statuses it wrote."""

    def __init__(self):
        super().__init__()
        self.statuses = []

    def ransac_lc_batch_dev(self, rp, rows_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, rec_out_ptr, T_out_ptr=None, n_assoc_out_ptr=None,
                            status_out_ptr=None, **kw):
        super().ransac_lc_batch_dev(rp, rows_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, rec_out_ptr, T_out_ptr, n_assoc_out_ptr, status_out_ptr, **kw)
        self.statuses.append(rl._view(status_out_ptr, (len(n1),), np.int32).copy())


@pytest.mark.parametrize("kind", CONFIGS)
def test_pools_path_equals_the_pair_loop(kind, built, orc):
    p, io, (pools, segs) = _config(kind, built)
    ctx = _Ctx(); reg = _ransac_reg(ctx)
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    want, subs = _pair_loop(orc, p, io, pools, segs)
    print(kind, "pairs registered:", len(got.timing_list), "calls:", ctx.ransacs, "associations:\n", want.clipper_num_associations)
    rl.assert_same_matrices(got, want)
    rl.assert_same_edges(got, want, subs)
    # one fused call over rows as the pool holds them, pass 1 and the removal as for any registration
    F = int(pools[0].pool.shape[1])
    assert ctx.ransacs == [(len(got.timing_list), F, True)] and ctx.tails == 1 and ctx.order[-2:] == ["ransac", "tail"] and "batch" not in ctx.order
    assert (ctx.order[0] == "boxes") == (kind == "aabb") and ("reduce" in ctx.order) == (kind == "self-shared-ids")
    assert F == (3 + 4 + D if kind == "mean-semantic-over-roman-pool" else 3)
    # the preconditions: pairs that reach the threshold, a pair that fails for want of associations
    st = _registered(want, ctx)
    assert (want.clipper_num_associations >= THRESH).sum() >= 2, "fewer than two pairs reach lc_association_thresh"
    assert ((st & _abi.ROMAN_ST_INSUFFICIENT) != 0).any(), "no registered pair fails with ROMAN_ST_INSUFFICIENT"
    assert len(got.lc_edges["pairs"]) >= 1
    if kind == "mean-semantic-over-roman-pool":
        assert (want.similarity_mat < 0.5).any() and (want.similarity_mat >= 0.5).any()
    if kind == "self-shared-ids":
        assert ((st & _abi.ROMAN_ST_EMPTY_MAP) != 0).any()      # a submap against itself keeps nothing


def _all_equal(a, b):
    for name in ("robots_nearby_mat", "clipper_num_associations", "T_ij_mat", "T_ij_hat_mat", "submap_yaw_diff_mat", "clipper_angle_mat", "clipper_dist_mat"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert all(np.array_equal(x, y) for ra, rb in zip(a.associated_objs_mat, b.associated_objs_mat) for x, y in zip(ra, rb))
    for k in ("pairs", "t", "q"):
        assert np.array_equal(a.lc_edges[k], b.lc_edges[k]), k


def test_a_pool_built_for_roman_registration_gives_what_a_ransac_pool_gives(built):
    """The stride: rows [x y z | 4 | d] and rows [x y z] of the same segments, no descriptor gate -> identical results."""
    p, io, _ = _config("radius-grid", built)
    res = []
    for kind in ("ransac", "roman"):
        ctx = _Ctx()
        res.append(sa.submap_align_pools(p, built[kind][0], io, registration=_ransac_reg(ctx)))
        assert ctx.ransacs[0][1] == (3 if kind == "ransac" else 3 + 4 + D)
    assert np.array_equal(built["ransac"][0][0].pool.numpy(), built["roman"][0][0].pool.numpy()[:, :3])
    _all_equal(res[0], res[1])
    assert (res[0].clipper_num_associations >= THRESH).sum() >= 2


def test_chunks_give_what_one_call_gives(built, monkeypatch):
    p, io, (pools, _) = _config("radius-grid", built)
    one_ctx = _Ctx()
    one = sa.submap_align_pools(p, pools, io, registration=_ransac_reg(one_ctx))
    B = len(one.timing_list)
    kmax = int(max(q.count.max() for q in pools)) ** 2
    per = -(-B // 3) - 1                                     # problems per chunk: at least 3 chunks
    assert per >= 1
    monkeypatch.setattr(sa, "RANSAC_ASSOC_CHUNK_BYTES", 8 * kmax * per)
    ctx = _Ctx()
    got = sa.submap_align_pools(p, pools, io, registration=_ransac_reg(ctx))
    assert len(ctx.ransacs) >= 3 and all(not tail for _, _, tail in ctx.ransacs) and sum(b for b, _, _ in ctx.ransacs) == B
    assert max(b for b, _, _ in ctx.ransacs) == per and ctx.tails == 1 and ctx.order[-1] == "tail" and ctx.order.count("tail") == 1
    _all_equal(got, one)


def test_refusals_name_the_other_way(built):
    p, io, (pools, _) = _config("radius-grid", built)

    def refused(pl, reg, text):
        with pytest.raises(ValueError, match="to_submaps") as e:
            sa.submap_align_pools(p, pl, io, registration=reg)
        assert text in str(e.value) and "submap_align_grid" in str(e.value)
    # pools of dim 2
    _, flat, _ = gg._pools("roman", None, dim=2)
    ctx = _Ctx()
    refused(flat, _ransac_reg(ctx), "no z")
    # a cap above ROMAN_RANSAC_MAX_OBJECTS
    refused([dataclasses.replace(pools[0], cap=_abi.ROMAN_RANSAC_MAX_OBJECTS + 1), pools[1]], _ransac_reg(ctx), str(_abi.ROMAN_RANSAC_MAX_OBJECTS))
    assert ctx.gates == 0 and ctx.aabb_gates == 0 and ctx.ransacs == [] and ctx.tails == 0 and ctx.order == []
    # a context without the call
    old = gg.PoolsStubContext(0)
    refused(pools, _ransac_reg(old), "roman_ransac_lc_batch_dev")
    assert old.gates == 0 and old.tails == 0 and old.calls == []
    # no context set, host tensors: nothing tries to make a HIP context
    reg = _ransac_reg()
    refused(pools, reg, "no context")
    assert reg._ctx is None


def test_factory_packs_centres_only():
    segs, _, _ = synth.make_map(20, D, seed=3, n_poses=8)
    table = MapTable.from_segments(RansacReg(), segs)
    assert table.feats.shape == (20, 3) and table.desc_dim == 0 and table.point_dim == 3
    assert np.array_equal(table.feats, np.array([np.asarray(s.center).reshape(-1)[:3] for s in segs]))
    assert np.array_equal(table.ids, [s.id for s in segs]) and table.times.shape == (20, 2)
    assert MapTable.from_segments(RansacReg(), []).feats.shape == (0, 3)


def test_run_lc_batch_dispatches_a_ransac_reg(orc):
    """run_lc_batch -> run_ransac_lc_batch -> Context.ransac_lc_batch with kmax = the largest n1 * n2, over rows of any width."""
    P, Q, _, _, _ = ro.planted(7, 6, 301, n_in=5)
    rows = np.full((13, 5), np.nan); rows[:7, :3] = P; rows[7:, :3] = Q
    batch = ab.AlignmentBatch(rows, np.array([0, 0], np.int64), np.array([7, 0], np.int32), np.array([7, 7], np.int64), np.array([6, 6], np.int32))
    seen = {}

    class Ctx(rl.RansacLcStubContext):
        def ransac_lc_batch(self, rp, rows, off1, n1, off2, n2, lc, kmax=None, counts=None):
            seen["kmax"] = kmax
            return super().ransac_lc_batch(rp, rows, off1, n1, off2, n2, lc, kmax, counts)
    lc = LcInputs(lc_association_thresh=THRESH)
    res = ab.run_lc_batch(_ransac_reg(), batch, lc, ctx=Ctx())
    assert seen["kmax"] == 42 and res.ransac_records is not None and np.all(res.stats["n_pass"] == 0)
    assert res.status.tolist() == [_abi.ROMAN_ST_OK, _abi.ROMAN_ST_EMPTY_MAP] and len(res.assoc[0]) == 5 and res.accepted.tolist() == [0]
    assert res.records["flags"].tolist() == [_abi.ROMAN_LC_ACCEPTED, _abi.ROMAN_LC_FAILED_INSUFFICIENT]
    with pytest.raises(ValueError, match="initial vector"):
        ab.run_lc_batch(_ransac_reg(), batch, lc, u0=np.zeros(3), ctx=Ctx())
