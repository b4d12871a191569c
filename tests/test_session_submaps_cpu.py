"""The submaps of every map of a session in one call without a GPU: build_session_pools over a stand-in context
whose session_submaps_dev is tests/_submaps_oracle.py per map, held field by field to build_submap_pool per robot; its refusals
before any context exists; and submap_align_session over the pools it leaves — the same results as over separately built copies,
on the session's own storage where the pools are its consecutive row ranges, through the concatenation everywhere else."""
import dataclasses

import numpy as np
import pytest

import _session as ss
import _session_submaps as sx
import _submaps_oracle as so
from roman_amd import synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import (FillSubmapParams, FrameTable, MapTable, SubmapParams, build_session_pools, build_submap_pool,
                                     submap_centers)

D = 16
VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None), dict(keep=0.8, first_pose=3, last_pose=None), dict(keep=0.9, first_pose=0, last_pose=19)]


def robots(R, params, empty_map=(), no_centers=(), semantic=True):
    """R robots' views of one place (tests/_session.robot_view: different N, different S, different rows) -> (registration, tables,
    centers).  A robot in `empty_map` has centres and a map without segments, one in `no_centers` a map and no centre."""
    reg = SubmapAlignParams(method="roman" if semantic else "gravity", semantics_dim=D).get_object_registration()
    base = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
    tables, centers = [], []
    for r in range(R):
        sg, traj, times = ss.robot_view(*base, r, **VIEWS[r])
        t = MapTable.from_segments(reg, sg)
        if r in empty_map:
            t = dataclasses.replace(t, feats=t.feats[:0].copy(), times=t.times[:0].copy(), ids=t.ids[:0].copy())
        if r in no_centers:
            traj, times = [], np.zeros(0)
        tables.append(t); centers.append(submap_centers(traj, times, params))
    return reg, tables, centers


def params_of(**kw):
    return SubmapParams(**{**dict(max_size=12, radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor='mean_semantic'), **kw})


CASES = [dict(name="one-robot", R=1, kw={}),
         dict(name="three-robots-empty-map-and-no-centres", R=3, kw={}, empty_map=(1,), no_centers=(2,)),
         dict(name="empty-in-front", R=3, kw=dict(pruning_method='time'), empty_map=(0,)),
         dict(name="time-pruning-window", R=3, kw=dict(pruning_method='time', time_threshold=50.0)),
         dict(name="no-max-size-cap", R=3, kw=dict(max_size=None, radius=15.0), cap=10),           # (slots shorter than the members: truncation)
         dict(name="no-max-size-whole-map", R=2, kw=dict(max_size=None, radius=8.0, submap_descriptor=None)),
         dict(name="no-descriptor-no-radius", R=3, kw=dict(submap_descriptor=None, radius=None, max_size=9), semantic=False)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_session_pools_equal_build_submap_pool_per_robot(case):
    params = params_of(**case["kw"])
    reg, tables, centers = robots(case["R"], params, case.get("empty_map", ()), case.get("no_centers", ()), case.get("semantic", True))
    assert len({len(t) for t in tables}) == case["R"] and (case["R"] == 1 or len({len(c) for c in centers}) > 1), "maps of one size"
    ctx = sx.OracleSessionSubmapContext()
    pools = build_session_pools(reg, tables, centers, params, ctx=ctx, device="cpu", cap=case.get("cap"))
    assert ctx.session_calls == 1 and ctx.syncs == 1 and ctx.calls == 0 and len(pools) == case["R"]
    cap = pools[0].cap
    assert cap == (params.max_size or case.get("cap") or max(len(t) for t in tables))
    for r, got in enumerate(pools):
        if len(tables[r]):
            sx.same_pool(got, build_submap_pool(reg, tables[r], centers[r], params, ctx=so.OracleSubmapContext(), device="cpu", cap=cap))
        else:                                                # (build_submap_pool does not take a map without segments: the cleared outputs, untouched)
            assert not got.count.any() and not got.status.any() and (got.src == -1).all() and (got.ids == -1).all() and len(got.count) == len(centers[r]) > 0
            assert not got.pool.numpy().any() and (got.ids_dev.numpy() == -1).all() and (got.desc is None or np.isnan(got.desc).all())
        assert tuple(got.pool.shape) == (len(centers[r]) * cap, tables[r].point_dim + tables[r].feats.shape[1] - 3)
        assert got.src[got.count > 0].max(initial=-1) < len(tables[r])                      # map-local indices
    live = [q for q, t, c in zip(pools, tables, centers) if len(t) and len(c)]
    assert all(len(q.nonempty) for q in live), "a robot with a map and centres has no non-empty submap: nothing was compared"
    for field in ("pool", "ids_dev") + (("desc_dev",) if params.submap_descriptor else ()):
        sx.one_storage(pools, field)
    if params.max_size is None:
        assert any((q.status == so.ST_TRUNCATED).any() for q in pools) == (case.get("cap") is not None)


def test_no_robots_make_no_context():
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    assert build_session_pools(reg, [], [], params_of()) == []


def test_refusals_come_before_a_context_is_made():
    params = params_of()
    reg, tables, centers = robots(3, params)
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    with pytest.raises(ValueError, match=r"build_submap_pool\(fill=\.\.\.\)"):
        build_session_pools(reg, tables, centers, params, fill=[[np.zeros(0, np.int32)]] * 3)
    with pytest.raises(ValueError, match=r"build_submap_pool\(fill=\.\.\.\)"):
        build_session_pools(reg, tables, centers, SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=True))
    with pytest.raises(ValueError, match=r"build_submap_pool\(fill=\.\.\.\)"):
        build_session_pools(reg, tables, centers, FillSubmapParams())
    t1 = tables[1]
    for other in (dataclasses.replace(t1, feats=np.ascontiguousarray(t1.feats[:, :-1])), dataclasses.replace(t1, point_dim=2),
                  dataclasses.replace(t1, desc_dim=D - 1), dataclasses.replace(t1, invariant=None)):
        with pytest.raises(ValueError, match="row width, point_dim, desc_dim or invariant"):
            build_session_pools(reg, [tables[0], other, tables[2]], centers, params)
    with pytest.raises(ValueError, match="one SubmapCenters per table"):
        build_session_pools(reg, tables, centers[:2], params)
    fr = FrameTable(np.zeros(4), np.zeros((4, 3)), np.zeros((4, 8)))
    with pytest.raises(ValueError, match="one FrameTable per table"):
        build_session_pools(reg, tables, centers, params_of(submap_descriptor='mean_frame_descriptor'), frames=[fr, fr])
    # ... and what build_submap_pool refuses per robot
    with pytest.raises(ValueError, match="needs the map's frames"):
        build_session_pools(reg, tables, centers, params_of(submap_descriptor='stacked_frame_descriptors'))
    with pytest.raises(ValueError, match="needs the map's frames"):
        build_session_pools(reg, tables, centers, params_of(submap_descriptor='mean_frame_descriptor'), frames=[fr, None, fr])
    with pytest.raises(ValueError, match="unknown submap_descriptor"):
        build_session_pools(reg, tables, centers, params_of(submap_descriptor='median'))
    with pytest.raises(ValueError, match="max_size must be None or >= 1"):
        build_session_pools(reg, tables, centers, params_of(max_size=0))
    bare = [dataclasses.replace(t, desc_dim=0) for t in tables]
    with pytest.raises(ValueError, match="needs a registration with semantic descriptors"):
        build_session_pools(reg, bare, centers, params)


# ---------------------------------------------------------------------------------------------
# submap_align_session over the pools of one build
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    params = params_of()
    reg, tables, centers = robots(3, params)
    pools = build_session_pools(reg, tables, centers, params, ctx=sx.OracleSessionSubmapContext(), device="cpu")
    apart = [build_submap_pool(reg, t, c, params, ctx=so.OracleSubmapContext(), device="cpu") for t, c in zip(tables, centers)]
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8,
                          single_robot_lc_time_thresh=40.0)
    return reg, pools, apart, p, sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)


def run(reg, p, io, pools, pairs):
    ctx = sx.RecordingSessionContext(); reg.set_context(ctx)
    ctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
    return sa.submap_align_session(p, pools, pairs, io, registration=reg), ctx


def equal_blocks(got, want):
    assert list(got) == list(want)
    aligned = 0
    for key in want:
        ss.compare(got[key], want[key])
        aligned += int((want[key].clipper_num_associations >= 4).sum())
    assert aligned >= 2, "hardly a pair aligned: the comparison would show nothing"


def test_session_runs_on_the_storage_of_one_build(built):
    reg, pools, apart, p, io = built
    cross = [(0, 1), (0, 2), (1, 2)]
    want, wctx = run(reg, p, io, apart, cross)
    got, gctx = run(reg, p, io, pools, cross)
    equal_blocks(got, want)
    first = sx.one_storage(pools, "pool")
    assert gctx.batch_pools and set(gctx.batch_pools) == {first}, "the batch did not read the session's own storage"
    assert not set(wctx.batch_pools) & {q.pool.data_ptr() for q in apart}, "separately built pools were not concatenated"


def test_self_blocks_read_the_ids_of_one_build(built):
    reg, pools, apart, p, io = built
    want, wctx = run(reg, p, io, apart, None)
    got, gctx = run(reg, p, io, pools, None)
    equal_blocks(got, want)
    assert gctx.order.count("reduce") == 1 and gctx.reduce_ids == [sx.one_storage(pools, "ids_dev")]
    assert gctx.reduce_rows == wctx.reduce_rows == [int(sum(q.pool.shape[0] for q in pools))]
    assert wctx.reduce_ids[0] not in {q.ids_dev.data_ptr() for q in apart}


@pytest.mark.parametrize("pick", [(0, 2), (1, 0), (0, 1, "apart")], ids=["gap", "other-order", "one-built-apart"])
def test_pools_that_are_not_one_run_of_rows_are_concatenated(built, pick):
    reg, pools, apart, p, io = built
    mine = [apart[1] if k == 1 and "apart" in pick else pools[k] for k in pick if k != "apart"]
    theirs = [apart[k] for k in pick if k != "apart"]
    cross = [(0, 1)]
    want, _ = run(reg, p, io, theirs, cross)
    got, gctx = run(reg, p, io, mine, cross)
    for key in want:
        ss.compare(got[key], want[key])
    assert gctx.batch_pools and not set(gctx.batch_pools) & {q.pool.data_ptr() for q in pools}, "the batch read a pool in place where it had to concatenate"


def test_one_storage_helper():
    import torch
    whole = torch.arange(60, dtype=torch.float64).reshape(12, 5)
    a, b, c = whole[:3], whole[3:7], whole[7:]
    v = sa._one_storage(torch, [a, b, c])
    assert v.data_ptr() == whole.data_ptr() and torch.equal(v, whole)
    v = sa._one_storage(torch, [b, c])
    assert v.data_ptr() == b.data_ptr() and torch.equal(v, whole[3:])
    for parts in ([a, c], [b, a], [a, b.clone()], [a], [a, None], [whole[:, :2], whole[:, 2:]], [a, whole[3:7, :4]]):
        assert sa._one_storage(torch, parts) is None
