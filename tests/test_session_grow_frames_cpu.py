"""grow_session_pools in the frame-descriptor modes with resident frame tables without a GPU: three robots over a
stand-in whose session_frame_select_list_dev is tests/_frame_desc_oracle.py per LISTED slot (tests/_session_grow_frames.py).  After
every step the pools equal build_session_pools over the same inputs field by field, `touched` is the brute-force difference to the
step before, only appended frames went up, one list call reselected, and the grown pools feed submap_align_session_update."""
import numpy as np
import pytest

import _session_grow_frames as gf
import _session_submaps as sx
import _session_update as su
import _session_update_stacked as sus
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align import submaps as sm
from roman_amd.align.submaps import FrameTable, SubmapParams, build_session_pools, grow_session_pools

D = gf.sg.D
MODES = [('mean_frame_descriptor', None), ('mean_frame_descriptor', 4.0), ('stacked_frame_descriptors', None), ('stacked_frame_descriptors', 4.0)]
IDS = ["mean", "mean-dist-ignored", "stacked", "stacked-thin"]


def params_of(mode, dist):
    return SubmapParams(max_size=40, radius=15.0, time_threshold=10.0, pruning_method='distance', submap_descriptor=mode, frame_descriptor_dist=dist)


def registration():
    return SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()


def fresh(reg, tables, centers, params, frames, cap):
    return build_session_pools(reg, tables, centers, params, ctx=gf.fresh_ctx(), device="cpu", cap=cap, frames=frames)


def check_pools(pools, want):
    for got, w in zip(pools, want):
        sx.same_pool(got, w)
        gf.same_frames(got, w)


@pytest.mark.parametrize("mode,dist", MODES, ids=IDS)
@pytest.mark.parametrize("growth", [1.5, 1.0], ids=["room", "tight"])
def test_grown_pools_equal_a_fresh_build_over_resident_frame_tables(mode, dist, growth, monkeypatch):
    """growth 1.0: no spare capacity — every step makes the tensors anew and the 64 -> 65 step lays the mask rows out at a new stride."""
    import torch
    monkeypatch.setattr(sm, "GROWTH", growth)
    params, reg = params_of(mode, dist), registration()
    session = gf.FrameSession(reg, params)
    stacked = mode == 'stacked_frame_descriptors'
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor=mode, frame_descriptor_dist=dist,
                          submap_descriptor_thresh=0.55, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    state, align_state, before, old_nf = None, sa.SessionAlignState(), None, [0, 0, 0]
    unlisted = by_span = 0
    for k in range(session.STEPS):
        tables, centers, frames = session.stage(k)
        ctx = gf.Ctx()
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", frames=frames)
        want = fresh(reg, tables, centers, params, frames, pools[1].cap)
        check_pools(pools, want)
        # one list call each, no per-robot selection, one synchronisation
        assert ctx.list_calls == 1 and len(ctx.frame_lists) == 1 and getattr(ctx, "frame_selects", 0) == 0 and ctx.syncs == 1
        nf = [len(f) for f in frames]
        assert state.frames_uploaded == sum(nf) - sum(old_nf) and state.frames_listed == len(ctx.frame_lists[0]) and state.n_frames == nf
        assert set(ctx.lists[0].tolist()) <= set(ctx.frame_lists[0].tolist())
        S = sum(len(q.count) for q in pools)
        if k == 0:
            assert ctx.frame_lists[0].tolist() == list(range(S)) and all(t.all() for t in touched)
        else:
            expect = gf.frame_differs(before, want)
            for r in range(3):
                assert touched[r].dtype == bool and np.array_equal(touched[r], expect[r]), (k, r, touched[r], expect[r])
            unlisted += S - state.frames_listed
            by_span += len(set(ctx.frame_lists[0].tolist()) - set(ctx.lists[0].tolist()))
        # the mask rows of a robot have room for its words; the views are strided where there is more
        rb = ctx.frame_robots
        assert rb["n_frames"].tolist() == nf and (rb["mask_words"] >= (rb["n_frames"] + 63) // 64).all() and rb["n_sub"].tolist() == [len(c) for c in centers]
        assert pools[1].frame_mask.shape[1] == (nf[1] + 63) // 64
        # one storage: the alignment reads the frame table in place
        live = [q.frame_desc_dev for q in pools[1:]]
        one = sa._one_storage(torch, live)
        assert one is not None and one.data_ptr() == live[0].data_ptr() and one.shape[0] == nf[1] + nf[2]
        if stacked:
            calls = []
            for call in (lambda: sa.submap_align_session_update(align_state, p, pools, touched, None, io, registration=reg),
                         lambda: sa.submap_align_session(p, want, None, io, registration=reg)):
                actx = sus.SessionUpdateStackedListStubContext(); reg.set_context(actx)
                actx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
                calls.append(call())
            assert list(calls[0]) == list(calls[1])
            for key in calls[1]:
                su.equal(calls[0][key], calls[1][key], sim_atol=1e-12)
        before, old_nf = want, nf
    assert unlisted >= 1, "every slot was reselected at every step: the frame list selected nothing"
    assert by_span >= 1, "no old slot was reselected for an appended frame alone: the span rule was not exercised"
    # the same inputs again: nothing is appended, nothing is listed, nothing changes
    ctx = gf.Ctx()
    pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", frames=frames)
    assert state.listed == 0 and state.frames_listed == 0 and state.frames_uploaded == 0 and ctx.frame_lists[0].tolist() == []
    assert not any(t.any() for t in touched)
    check_pools(pools, want)
    # frames_changed: the robot's table goes up whole and all its submaps are listed — and found unchanged
    ctx = gf.Ctx()
    pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", frames=frames, frames_changed=[False, False, True])
    lo = len(centers[1])
    assert ctx.frame_lists[0].tolist() == list(range(lo, lo + len(centers[2]))) and state.frames_uploaded == len(frames[2]) and state.listed == 0
    assert not any(t.any() for t in touched)
    check_pools(pools, want)
    # ... with other descriptors in it: the means follow (the masks do not depend on them)
    other = FrameTable(frames[2].times, frames[2].pos, frames[2].desc + 1.0)
    frames2 = [frames[0], frames[1], other]
    pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=frames2, frames_changed=[False, False, True])
    want2 = fresh(reg, tables, centers, params, frames2, pools[1].cap)
    check_pools(pools, want2)
    expect = gf.frame_differs(want, want2)
    for r in range(3):
        assert np.array_equal(touched[r], expect[r]), r
    assert touched[2].any() == (not stacked)


def test_a_context_without_the_entry_takes_the_per_robot_path():
    params, reg = params_of('mean_frame_descriptor', None), registration()
    session = gf.FrameSession(reg, params)
    state, before = None, None
    assert not hasattr(gf.OldCtx, "session_frame_select_list_dev")
    for k in range(session.STEPS):
        tables, centers, frames = session.stage(k)
        ctx = gf.OldCtx()
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device="cpu", frames=frames)
        want = fresh(reg, tables, centers, params, frames, pools[1].cap)
        check_pools(pools, want)
        assert ctx.frame_selects == 2 and state.n_frames is None and "f_mask" not in state.t       # (robot 0 has no submap: no call for it)
        if before is not None:
            expect = gf.frame_differs(before, want)
            for r in range(3):
                assert np.array_equal(touched[r], expect[r]), (k, r)
        before = want


def test_refusals():
    params, reg = params_of('stacked_frame_descriptors', 4.0), registration()
    session = gf.FrameSession(reg, params)
    tables, centers, frames = session.stage(1)
    _, _, state = grow_session_pools(None, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=frames)
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    earlier = session.stage(0)[2]
    with pytest.raises(ValueError, match="frame table shrank"):
        grow_session_pools(state, reg, tables, centers, params, frames=[frames[0], earlier[1], frames[2]])
    for bad in ([True], [False] * 4):
        with pytest.raises(ValueError, match="frames_changed"):
            grow_session_pools(state, reg, tables, centers, params, frames=frames, frames_changed=bad)
    # a non-empty submap whose span holds no frame: the reference cannot build its descriptor
    far = FrameTable(frames[2].times + 1e6, frames[2].pos, frames[2].desc)
    with pytest.raises(ValueError, match="no frame of the map lies in its time span"):
        grow_session_pools(None, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=[frames[0], frames[1], far])


def test_a_state_stays_with_its_kind_of_context_and_ends_with_a_call_that_raised():
    params, reg = params_of('stacked_frame_descriptors', 4.0), registration()
    session = gf.FrameSession(reg, params)
    tables, centers, frames = session.stage(0)
    _, _, state = grow_session_pools(None, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=frames)
    layout = (list(state.n_sub), list(state.n_frames), list(state.mask_words), {k: v.clone() for k, v in state.t.items()})
    tables, centers, frames = session.stage(1)
    # resident frame tables, then a context without the entry: refused before anything moves, the state serves on
    with pytest.raises(ValueError, match="no session_frame_select_list_dev"):
        grow_session_pools(state, reg, tables, centers, params, ctx=gf.OldCtx(), device="cpu", frames=frames)
    assert not state.unfinished and (state.n_sub, state.n_frames, state.mask_words) == layout[:3]
    assert all(np.array_equal(v.numpy(), state.t[k].numpy(), equal_nan=True) for k, v in layout[3].items())
    pools, _, state = grow_session_pools(state, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=frames)
    check_pools(pools, fresh(reg, tables, centers, params, frames, pools[1].cap))
    # a call that raises behind the device call has moved the tensors: nothing of the new layout is recorded and the state is refused
    tables, centers, frames = session.stage(2)
    n_frames, n_sub = list(state.n_frames), list(state.n_sub)
    far = FrameTable(frames[2].times + 1e6, frames[2].pos, frames[2].desc)
    with pytest.raises(ValueError, match="no frame of the map lies in its time span"):
        grow_session_pools(state, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=[frames[0], frames[1], far], frames_changed=[False, False, True])
    assert state.unfinished and state.n_frames == n_frames and state.n_sub == n_sub
    with pytest.raises(ValueError, match="begin again with a new state"):
        grow_session_pools(state, reg, tables, centers, params, ctx=gf.Ctx(), device="cpu", frames=frames)
