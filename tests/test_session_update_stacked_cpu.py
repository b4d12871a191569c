"""submap_align_session_update with 'stacked_frame_descriptors' over the pair list without a GPU: a session that
grows in steps over a stand-in context with roman_session_stacked_sim_list_dev, after every step equal to submap_align_session
over the same pools on the same stand-in.  The stand-in leaves NaN in every entry of the dense similarity that is not listed, so
a gate that read one would show it; the first call lists everything and takes the whole-block call."""
import numpy as np

import _session_update as su
import _session_update_stacked as sus
import test_session_stacked_cpu as ts
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from test_session_cpu import gt_for

STEPS = 3       # a first call and two appending steps


def grow(stand_in):
    """The pools of tests/test_session_stacked_cpu.py, R = 3 with an empty robot (1) and a robot without frames (2), all r <= s:
    every robot's submaps but the last two, then one more per step.  Yields (step, update context, update results, full results)."""
    reg, final = ts.make_pools(3, empty=(1,), no_frames=(2,))
    assert min(len(q.count) for q in final) >= STEPS + 1
    p = SubmapAlignParams(method="roman", semantics_dim=ts.D, submap_radius=15.0, submap_descriptor=ts.MODE, frame_descriptor_dist=10.0,
                          submap_descriptor_thresh=ts.THRESH, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    gt_final = [gt_for(final[0], 70), None, None]
    state = sa.SessionAlignState()
    for step in range(STEPS):
        pools = [su.pool_prefix(q, len(q.count) - (STEPS - 1) + step) for q in final]
        gt = [None if g is None else g[:len(q.count)] for g, q in zip(gt_final, pools)]
        calls = []
        for call in (lambda: sa.submap_align_session_update(state, p, pools, None, None, io, registration=reg, gt_poses=gt),
                     lambda: sa.submap_align_session(p, pools, None, io, registration=reg, gt_poses=gt)):
            ctx = stand_in(); reg.set_context(ctx)
            ctx.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
            calls.append((ctx, call()))
        yield step, calls[0][0], calls[0][1], calls[1][1]


def test_the_similarity_follows_the_pair_list_after_the_first_call():
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    decided, listed_fewer = False, 0
    for step, ctx, got, want in grow(sus.SessionUpdateStackedListStubContext):
        assert list(got) == list(want) == blocks
        for key in blocks:
            su.equal(got[key], want[key], sim_atol=1e-12)
        decided = decided or ts.gated_and_todo(want, ts.THRESH)
        assert len(ctx.lists) == 1 and ctx.session_gates == 0
        if step == 0:                                        # everything is listed: the whole-block call, as before
            assert ctx.order[:2] == ["session_stacked_sim", "session_gate_list"] and ctx.session_stacked_sims == 1 and ctx.sim_lists == []
            assert len(ctx.lists[0]) == ctx.totals[0]
        else:
            assert ctx.order[:2] == ["session_stacked_sim_list", "session_gate_list"] and ctx.session_stacked_sims == 0
            assert ctx.order.count("session_stacked_sim_list") == 1 and len(ctx.sim_lists) == 1
            assert ctx.sim_lists[0].dtype == ctx.lists[0].dtype and np.array_equal(ctx.sim_lists[0], ctx.lists[0])      # one list for both calls
            assert 0 < len(ctx.lists[0]) < ctx.totals[0]
            listed_fewer += 1
    assert listed_fewer == STEPS - 1
    assert decided, "no block holds a GATED and a TODO pair: the similarity decides nothing"


def test_a_context_without_the_list_entry_takes_the_whole_block_call():
    assert not hasattr(su.SessionUpdateStackedStubContext, "session_stacked_sim_list_dev")
    for step, ctx, got, want in grow(su.SessionUpdateStackedStubContext):
        for key in want:
            su.equal(got[key], want[key], sim_atol=1e-12)
        assert ctx.order[:2] == ["session_stacked_sim", "session_gate_list"] and ctx.session_stacked_sims == 1
        assert (len(ctx.lists[0]) == ctx.totals[0]) == (step == 0)
