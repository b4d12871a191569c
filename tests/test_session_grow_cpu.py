"""grow_session_pools without a GPU: a session that grows in steps over a stand-in context whose
session_submaps_list_dev is tests/_submaps_oracle.py per listed submap (tests/_session_grow.py).  After every step the pools equal
build_session_pools over the same inputs field by field and byte for byte, `touched` is exactly the set of slots that differ between
the two consecutive fresh builds (plus the new ones), the pools are adjacent ranges of one storage, and
submap_align_session_update(touched=touched) over them equals submap_align_session over the fresh build."""
import dataclasses

import numpy as np
import pytest

import _session as ss
import _session_grow as sg
import _session_submaps as sx
import _session_update as su
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import (FillSubmapParams, FrameTable, SessionPoolsState, SubmapParams, build_session_pools, grow_session_pools)

D = sg.D
STEPS = 5                                                                    # a first call and four growth steps


def params_of(**kw):
    return SubmapParams(**{**dict(max_size=40, radius=15.0, time_threshold=10.0, pruning_method='distance', submap_descriptor='mean_semantic'), **kw})


def registration():
    return SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()


def fresh(reg, tables, centers, params, cap):
    return build_session_pools(reg, tables, centers, params, ctx=sx.OracleSessionSubmapContext(), device="cpu", cap=cap)


def plan_edits(session, pools, k):
    """The rewrites of stage k, decided on the fresh pools of stage k - 1 -> changed_rows.  Stage 2: a member of an old submap of
    robot 0 that is not full leaves the place (the submap SHRINKS: the pad contract).  Stage 3: the last robot's row 1 is seen
    again later (times only)."""
    R = session.R
    rows = [None] * R
    if k == 2:
        q = pools[0]
        s = int(np.nonzero((q.count > 1) & (q.count < q.cap))[0][0])
        row = int(q.src[s, 0])
        session.edit(0, row, feats=session.full[0].feats[row, :3] + 1000.0)
        rows[0] = [row]
    if k == 3:
        r = R - 1
        t = session.full[r].times[1].copy()
        session.edit(r, 1, times=[t[0], t[1] + 7.0])
        rows[r] = np.array([1])
    return rows


@pytest.mark.parametrize("R,kw", [(1, {}), (3, {}), (3, dict(max_size=None, pruning_method='time', submap_descriptor=None))], ids=["R1", "R3", "R3-no-max-size"])
def test_grown_pools_equal_a_fresh_build_and_touched_is_what_differs(R, kw):
    params = params_of(**kw)
    reg = registration()
    session = sg.GrowingSession(reg, R, params, STEPS)
    cap = 30 if params.max_size is None else None
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor=params.submap_descriptor, submap_descriptor_thresh=0.8,
                          single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    state, align_state, before = None, sa.SessionAlignState(), None
    shrank = unlisted = aligned = 0
    for k in range(STEPS):
        rows = plan_edits(session, before, k) if k else None
        tables, centers = session.stage(k)
        ctx = sg.OracleSessionListContext()
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", cap=cap, changed_rows=rows)
        want = fresh(reg, tables, centers, params, pools[0].cap)
        assert ctx.list_calls == 1 and ctx.session_calls == 0 and ctx.syncs == 1
        for got, w in zip(pools, want):
            sx.same_pool(got, w)
        for field in ("pool", "ids_dev") + (("desc_dev",) if params.submap_descriptor else ()):
            sx.one_storage(pools, field)
        if R > 1:
            import torch
            assert sa._one_storage(torch, [q.pool for q in pools]).data_ptr() == pools[0].pool.data_ptr()
        # touched: everything at the first call; afterwards the new submaps and exactly the old ones that differ between the fresh builds
        expect = [np.ones(len(w.count), dtype=bool) for w in want] if k == 0 else sg.differing_slots(before, want)
        for r in range(R):
            assert touched[r].dtype == bool and np.array_equal(touched[r], expect[r]), (k, r, touched[r], expect[r])
        S = sum(len(q.count) for q in pools)
        assert state.total == S and state.listed == len(ctx.lists[0]) and (k > 0 or state.listed == S)
        if k:
            old = sum(len(q.count) for q in before)
            unlisted += S - state.listed
            shrank += int(sum((w.count[:len(b.count)] < b.count).sum() for w, b in zip(want, before)))
            assert state.listed >= S - old
            # the former last submap of every robot is listed: its t_hi moved
            for r in range(R):
                assert int(np.cumsum([0] + [len(q.count) for q in pools])[r]) + len(before[r].count) - 1 in ctx.lists[0].tolist()
        # into the alignment: the growing call with `touched` against the full call over the fresh build
        uctx = su.SessionUpdateStubContext(); reg.set_context(uctx)
        uctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
        got_lc = sa.submap_align_session_update(align_state, p, pools, touched, None, io, registration=reg)
        fctx = ss.SessionStubContext(); reg.set_context(fctx)
        fctx.n_objects = uctx.n_objects
        want_lc = sa.submap_align_session(p, want, None, io, registration=reg)
        assert list(got_lc) == list(want_lc)
        for key in want_lc:
            su.equal(got_lc[key], want_lc[key], sim_atol=1e-12)
            aligned += int((want_lc[key].clipper_num_associations >= 4).sum())
        before = want
    assert shrank >= 1, "no old submap lost a row: the pad contract was not exercised"
    assert unlisted >= 1, "every submap was listed at every step: the list rule selected nothing"
    assert aligned >= 2 or R == 1, "hardly a pair aligned: the comparison would show nothing"      # (one robot: its self block only)
    # the same inputs again: nothing new, and whatever is listed again reports no change
    tables, centers = session.stage(STEPS - 1)
    ctx = sg.OracleSessionListContext()
    pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", cap=cap, rebuild='all')
    assert state.listed == state.total and not any(t.any() for t in touched)
    for got, w in zip(pools, fresh(reg, tables, centers, params, pools[0].cap)):
        sx.same_pool(got, w)


def test_rebuild_names_submaps_and_capacity_grows_in_place():
    params = params_of()
    reg = registration()
    session = sg.GrowingSession(reg, 3, params, STEPS)
    state, ptrs = None, []
    for k in range(STEPS):
        tables, centers = session.stage(k)
        ctx = sg.OracleSessionListContext()
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", rebuild=[[0], None, None] if k else None)
        ptrs.append(state.t["pool"].data_ptr())
        if k:
            assert 0 in ctx.lists[0].tolist() and not touched[0][0]                    # rebuilt on request, found unchanged
        for got, w in zip(pools, fresh(reg, tables, centers, params, pools[0].cap)):
            sx.same_pool(got, w)
    assert len(set(ptrs)) < len(ptrs), "the tensors were made anew at every step: no capacity was kept"
    assert state.t["pool"].shape[0] >= sum(len(c) for c in centers) * pools[0].cap


def test_frame_descriptor_modes_follow_the_fresh_build():
    """mean_frame_descriptor: frame_select_dev per robot behind the list call, as build_session_pools runs it; a submap whose frames
    changed is touched although its rows are not."""
    import _frame_desc_oracle as fo

    class Ctx(fo.FrameCallsMixin, sg.OracleSessionListContext):
        pass

    params = params_of(submap_descriptor='mean_frame_descriptor')
    reg = registration()
    session = sg.GrowingSession(reg, 2, params, 3)
    state, before = None, None
    for k in range(3):
        tables, centers = session.stage(k)
        frames = []
        for r in range(2):
            traj, times = session.traj[r]
            n = len(times) if k == 2 else int(session.starts[r][len(session.starts[r]) - (2 - k)])
            frames.append(FrameTable.from_map(traj[:n], times[:n], np.random.default_rng(9 + r).standard_normal((len(times), 8))[:n]))
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=Ctx(), device="cpu", frames=frames)
        want = build_session_pools(reg, tables, centers, params, ctx=type("F", (fo.FrameCallsMixin, sx.OracleSessionSubmapContext), {})(), device="cpu", frames=frames)
        for got, w in zip(pools, want):
            sx.same_pool(got, w)
            assert np.array_equal(got.frame_n, w.frame_n) and np.array_equal(got.frame_mask.numpy(), w.frame_mask.numpy())
        if before is not None:
            for r in range(2):
                m = len(before[r].count)
                W = want[r].frame_mask.shape[1]
                old_mask = np.zeros((m, W), np.int64); old_mask[:, :before[r].frame_mask.shape[1]] = before[r].frame_mask.numpy()
                differs = (old_mask != want[r].frame_mask.numpy()[:m]).any(axis=1) | (before[r].frame_n != want[r].frame_n[:m]) | \
                    (before[r].desc.view(np.int64) != want[r].desc[:m].view(np.int64)).any(axis=1)
                rows = sg.differing_slots([dataclasses.replace(before[r], desc=None)], [dataclasses.replace(want[r], desc=None)])[0]
                assert np.array_equal(touched[r], rows | np.concatenate([differs, np.ones(len(rows) - m, bool)])), (k, r)
        before = want


def test_refusals_come_before_a_context_is_made():
    params = params_of()
    reg = registration()
    session = sg.GrowingSession(reg, 3, params, STEPS)
    tables, centers = session.stage(1)
    _, _, state = grow_session_pools(None, reg, tables, centers, params, ctx=sg.OracleSessionListContext(), device="cpu")
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    grow = lambda st, tb=tables, cn=centers, prm=params, **kw: grow_session_pools(st, reg, tb, cn, prm, **kw)
    # what build_session_pools refuses, the force-fill mode included
    with pytest.raises(ValueError, match=r"build_submap_pool\(fill=\.\.\.\)"):
        grow(None, prm=FillSubmapParams())
    with pytest.raises(ValueError, match=r"build_submap_pool\(fill=\.\.\.\)"):
        grow(None, prm=SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=True))
    with pytest.raises(ValueError, match="one SubmapCenters per table"):
        grow(None, cn=centers[:2])
    with pytest.raises(ValueError, match="needs the map's frames"):
        grow(None, prm=params_of(submap_descriptor='stacked_frame_descriptors'))
    with pytest.raises(ValueError, match="unknown submap_descriptor"):
        grow(None, prm=params_of(submap_descriptor='median'))
    t1 = tables[1]
    with pytest.raises(ValueError, match="row width, point_dim, desc_dim or invariant"):
        grow(None, tb=[tables[0], dataclasses.replace(t1, point_dim=2), tables[2]])
    # another session than the state's
    with pytest.raises(ValueError, match="SessionPoolsState"):
        grow(state, tb=tables[:2], cn=centers[:2])                                    # robot count
    with pytest.raises(ValueError, match="SessionPoolsState"):
        grow(state, prm=params_of(max_size=12))                                       # cap
    with pytest.raises(ValueError, match="SessionPoolsState"):
        grow(state, prm=params_of(submap_descriptor=None))                            # submap_descriptor
    with pytest.raises(ValueError, match="SessionPoolsState"):
        grow(state, tb=[dataclasses.replace(t, point_dim=2) for t in tables])        # row layout
    # what only a growing session can get wrong
    earlier = session.stage(0)
    with pytest.raises(ValueError, match="shrank"):
        grow(state, tb=[earlier[0][0], tables[1], tables[2]])
    with pytest.raises(ValueError, match="shrank"):
        grow(state, cn=[centers[0], earlier[1][1], centers[2]])
    for bad in ([[len(tables[0])], None, None], [None, [-1], None], [None, None]):
        with pytest.raises(ValueError, match="changed_rows"):
            grow(state, changed_rows=bad)
    with pytest.raises(ValueError, match="rebuild"):
        grow(state, rebuild=[[len(centers[0])], None, None])
    assert isinstance(state, SessionPoolsState)


def test_no_robots_make_no_context():
    reg = registration()
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    pools, touched, state = grow_session_pools(None, reg, [], [], params_of())
    assert pools == [] and touched == [] and isinstance(state, SessionPoolsState)
