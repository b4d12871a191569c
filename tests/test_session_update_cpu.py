"""submap_align_session_update without a GPU: a session that grows in steps over a stand-in context, after every
step equal to submap_align_session over the same pools on the same stand-in — and the list the gate is handed holds exactly the
pairs with a touched side, so a version that lists everything does not pass."""
import dataclasses

import numpy as np
import pytest

import _session as ss
import _session_update as su
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from test_session_cpu import D, alternating_pose, gt_for, make_pools


def full_call(p, io, reg, pools, pairs, gt):
    ctx = ss.SessionStubContext(); reg.set_context(ctx)
    ctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
    return sa.submap_align_session(p, pools, pairs, io, registration=reg, gt_poses=gt)


def update_call(state, p, io, reg, pools, pairs, gt, touched=None):
    ctx = su.SessionUpdateStubContext(); reg.set_context(ctx)
    ctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
    return ctx, sa.submap_align_session_update(state, p, pools, touched, pairs, io, registration=reg, gt_poses=gt)


def expected_list(pools, blocks, flags):
    """The pairs with a touched side, block-local over the non-empty submaps, written out independently of runtime.session_pair_list."""
    out = []
    for b, (r, s) in enumerate(blocks):
        fi, fj = flags[r][pools[r].nonempty], flags[s][pools[s].nonempty]
        out += [(b, i, j) for i in range(len(fi)) for j in range(len(fj)) if fi[i] or fj[j]]
    return out


@pytest.mark.parametrize("desc,gt_on", [('mean_semantic', ()), (None, (0,)), ('mean_semantic', (0, 1, 2))], ids=["desc-no-gt", "no-desc-gt-on-one", "desc-gt-on-all"])
def test_update_equals_the_full_session_call_after_every_step(desc, gt_on):
    """Three robots, robot 1 without a segment (its blocks are empty), all r <= s: the self blocks drop shared segments.  A full
    first call, then three appending steps; submap `late` of robot 0 holds nothing until step 2; at step 3 the caller takes a
    segment out of an old submap of robot 2 — nothing the host-side inputs show — and flags it."""
    reg, final = make_pools(desc, 3, empty=(1,))
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor=desc, submap_descriptor_thresh=0.8,
                          single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    n = [len(q.count) for q in final]
    assert min(n) >= 5, n
    late = int(final[0].nonempty[1])
    changed = int(final[2].nonempty[0])
    gt_final = [gt_for(final[r], 70 + r) if r in gt_on else None for r in range(3)]
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    state = sa.SessionAlignState()
    before, aligned = None, 0
    for step in range(4):
        k = [m - 3 + step for m in n]
        pools = [su.pool_prefix(q, k[r], blank=(late,) if r == 0 and step < 2 else ()) for r, q in enumerate(final)]
        touched = None
        if step == 3:
            cnt = pools[2].count.copy(); cnt[changed] -= 1
            pools[2] = dataclasses.replace(pools[2], count=cnt)
            touched = [None, None, np.arange(k[2]) == changed]
        gt = [None if g is None else g[:k[r]] for r, g in enumerate(gt_final)]
        ctx, got = update_call(state, p, io, reg, pools, None, gt if gt_on else None, touched)
        want = full_call(p, io, reg, pools, None, gt if gt_on else None)
        assert list(got) == list(want) == blocks
        for key in blocks:
            su.equal(got[key], want[key], sim_atol=1e-12)
            aligned += int((want[key].clipper_num_associations >= 4).sum())
        # the list: only pairs with a touched side
        flags = [np.ones(m, dtype=bool) if step == 0 else np.arange(m) >= before[r] for r, m in enumerate(k)]
        if step == 2:
            flags[0][late] = True
        if step == 3:
            flags[2][changed] = True
        assert len(ctx.lists) == 1 and [tuple(x) for x in ctx.lists[0].tolist()] == expected_list(pools, blocks, flags), step
        assert (len(ctx.lists[0]) == ctx.totals[0]) == (step == 0) and state.listed == len(ctx.lists[0]) and state.total == ctx.totals[0]
        assert ctx.order[0] == "session_gate_list" and ctx.session_gates == 0 and ctx.order.count("reduce") <= 1
        before = k
    assert aligned >= 4, "hardly a pair aligned: the comparison would show nothing"
    # a call that touches nothing makes no context and returns the same
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    again = sa.submap_align_session_update(state, p, pools, None, None, io, registration=reg, gt_poses=gt if gt_on else None)
    for key in blocks:
        su.equal(again[key], want[key], sim_atol=1e-12)


@pytest.mark.parametrize("mode", ["aabb", "stacked"])
def test_update_equals_the_full_session_call_behind_boxes_and_stacked_similarity(mode):
    """The bounding-box gate (the pools of tests/test_session_aabb_cpu.py: robots 0 and 2 force-filled, robot 1 cut by radius, a
    descriptor, ground truth on robot 0) and stacked frame descriptors (the pools of tests/test_session_stacked_cpu.py): a full
    first call over every robot's submaps but the last, then one appending step — after each, every block equals
    submap_align_session on the same stand-in, and the call the mode needs comes first on the context."""
    import test_session_aabb_cpu as ta
    import test_session_stacked_cpu as ts
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    base = dict(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor_thresh=0.8, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    if mode == "aabb":
        reg, final = make_pools('mean_semantic', 3)
        for r in (0, 2):
            final[r] = ta.fill_pool(reg, r, 'mean_semantic')
        p = SubmapAlignParams(**base, force_fill_submaps=True, submap_descriptor='mean_semantic')
        stand_in, first_call, gt_final = su.SessionUpdateAabbStubContext, "session_boxes", [gt_for(final[0], 70), None, None]
    else:
        reg, final = ts.make_pools(3)
        p = SubmapAlignParams(**base, submap_descriptor=ts.MODE, frame_descriptor_dist=10.0)
        stand_in, first_call, gt_final = su.SessionUpdateStackedStubContext, "session_stacked_sim", [None] * 3
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    state = sa.SessionAlignState()
    aligned, decided = 0, False
    for step in range(2):
        pools = [su.pool_prefix(q, len(q.count) - 1 + step) for q in final]
        gt = [None if g is None else g[:len(q.count)] for g, q in zip(gt_final, pools)]
        calls = []
        for call in (lambda: sa.submap_align_session_update(state, p, pools, None, None, io, registration=reg, gt_poses=gt),
                     lambda: sa.submap_align_session(p, pools, None, io, registration=reg, gt_poses=gt)):
            ctx = stand_in(); reg.set_context(ctx)
            ctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
            calls.append((ctx, call()))
        (ctx, got), (full_ctx, want) = calls
        assert list(got) == list(want) == blocks
        for key in blocks:
            su.equal(got[key], want[key], sim_atol=1e-12)
            aligned += int((want[key].clipper_num_associations >= 4).sum())
        decided = decided or ts.gated_and_todo(want, 0.8)
        assert ctx.order[0] == full_ctx.order[0] == first_call and ctx.order[1] == "session_gate_list"
        assert ctx.session_gates == 0 and getattr(ctx, "session_aabb_gates", 0) == 0
        assert len(ctx.lists) == 1 and (len(ctx.lists[0]) == ctx.totals[0]) == (step == 0), step      # the step lists the pairs of the new submaps only
    assert aligned >= 4, "hardly a pair aligned: the comparison would show nothing"
    assert decided, "no block holds a GATED and a TODO pair: the similarity decides nothing"


def test_a_partner_going_from_odd_to_even_touches_the_whole_alternating_robot():
    """Robot 0's poses alternate under flattening (tests/test_session_cpu.py): when robot 1 grows from one submap to two, the pose
    robot 0's submaps are read with changes although none of its inputs did — all of robot 0 is listed again, in every block."""
    reg, pools = make_pools(None, 3)
    c = pools[0].centers
    pools[0] = dataclasses.replace(pools[0], centers=dataclasses.replace(c, pose_flu=np.stack([alternating_pose(T[:3, 3]) for T in c.pose_flu])))
    keep1 = pools[1].nonempty
    steps = []
    for live in (1, 2):
        cnt = pools[1].count.copy(); cnt[keep1[live:]] = 0
        steps.append([pools[0], dataclasses.replace(pools[1], count=cnt), pools[2]])
    assert len(pools[2].nonempty) % 2 == 0
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    blocks = [(0, 1), (0, 2), (2, 0)]
    state = sa.SessionAlignState()
    for k, pl in enumerate(steps):
        ctx, got = update_call(state, p, io, reg, pl, blocks, None)
        want = full_call(p, io, reg, pl, blocks, None)
        for key in blocks:
            su.equal(got[key], want[key], sim_atol=1e-12)
    n0, n2 = len(pools[0].nonempty), len(pools[2].nonempty)              # (growth that lists the new submaps' pairs only: the test above)
    assert len(ctx.lists[0]) == ctx.totals[0] == n0 * 2 + 2 * n0 * n2          # every pair has a submap of robot 0 on one side


def test_update_refuses_before_a_context_is_made():
    reg, pools = make_pools('mean_semantic', 2)
    base = dict(method="roman", semantics_dim=D, submap_radius=15.0)
    p, io = SubmapAlignParams(**base, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8), sa.SubmapAlignIO()
    state = sa.SessionAlignState()
    update_call(state, p, io, reg, pools, None, None)
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    upd = lambda st, prm, pl, touched=None, pairs=None, **kw: sa.submap_align_session_update(st, prm, pl, touched, pairs, io, registration=reg, **kw)
    n = [len(q.count) for q in pools]
    with pytest.raises(ValueError, match="shrank"):
        upd(state, p, [su.pool_prefix(pools[0], n[0] - 1), pools[1]])
    for bad in ([None], [np.zeros(n[0] + 1, bool), None], [None, np.zeros(n[1] - 1, bool)]):
        with pytest.raises(ValueError, match="touched"):
            upd(state, p, pools, bad)
    with pytest.raises(ValueError, match="SessionAlignState"):
        upd(state, p, pools, None, [(0, 1)])                                         # other robot_pairs
    with pytest.raises(ValueError, match="SessionAlignState"):
        upd(state, SubmapAlignParams(**base), pools)                                # another descriptor mode
    with pytest.raises(ValueError, match="SessionAlignState"):
        upd(state, SubmapAlignParams(**{**base, "method": "gravity"}, submap_descriptor='mean_semantic'), pools)       # another method
    with pytest.raises(ValueError, match="SessionAlignState"):
        upd(state, p, pools, gt_poses=[gt_for(pools[0], 1), None])                  # another ground-truth pattern
    # what submap_align_session refuses, with its words (the registration has no context set, as in tests/test_session_cpu.py)
    reg._ctx = None
    import torch
    wide = dataclasses.replace(pools[1], pool=torch.cat([pools[1].pool, pools[1].pool[:, :1]], dim=1))
    no_ids = dataclasses.replace(pools[0], ids_dev=None)
    _, bare = make_pools(None, 2)
    for prm, pl, pairs, what in ((p, [pools[0], wide], None, "row widths"), (p, [no_ids, pools[1]], None, "ids_dev"), (p, pools, [(0, 2)], "robot_pairs"),
                                 (p, pools, [(0, 1), (0, 1)], "robot_pairs"), (p, bare, None, "mean_semantic"),
                                 (SubmapAlignParams(**base, force_fill_submaps=True), pools, None, "bounding boxes"),
                                 (SubmapAlignParams(**base, submap_descriptor='stacked_frame_descriptors'), pools, None, "stacked_frame_descriptors")):
        with pytest.raises(ValueError, match="submap_align_pools") as e:
            upd(sa.SessionAlignState(), prm, pl, None, pairs)
        assert what in str(e.value), (what, str(e.value))
    with pytest.raises(ValueError, match="submap_align_pools"):
        upd(sa.SessionAlignState(), p, pools, gt_poses=[None])
