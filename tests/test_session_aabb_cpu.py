"""The session call in AABB mode (force_fill_submaps / no submap_radius) and with a RansacReg without a GPU:
submap_align_session over the stand-in of tests/_session_aabb.py against submap_align_pools called per block on the same pools
with the same stand-in — EXACTLY: both go through the same NumPy restatements on the same inputs."""
import dataclasses

import numpy as np
import pytest

import _fill_boxes_oracle as fo
import _self_pools as sp
import _session as ss
import _session_aabb as sx
import _submaps_oracle as so
import test_grid_gate_cpu as gg
import test_ransac_lc_cpu as trl
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import FillSubmapParams, MapTable, build_submap_pool, fill_centers
from test_session_cpu import D, alternating_pose, gt_for, make_pools, per_block


def fill_pool(reg, r, descriptor):
    """Robot r's own view of the place of test_session_cpu.make_pools, cut into force-fill slices."""
    base = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
    sg, traj, times = ss.robot_view(*base, r, keep=(1.0, 0.8, 0.9)[r], first_pose=(0, 3, 0)[r])
    table = MapTable.from_segments(reg, sg)
    fp = FillSubmapParams((12, 10, 14)[r], 6, descriptor)
    centers, slices = fill_centers(table, traj, times, fp)
    return build_submap_pool(reg, table, centers, fp, ctx=fo.OracleFillContext(), device="cpu", fill=slices)


def run_both(p, io, reg, pools, pairs, gt):
    R = len(pools)
    blocks = pairs or [(r, s) for r in range(R) for s in range(r, R)]
    ctx = sx.SessionAabbStubContext(); reg.set_context(ctx)
    want = per_block(p, io, reg, pools, blocks, gt)
    ctx2 = sx.SessionAabbStubContext(); reg.set_context(ctx2)
    ctx2.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
    got = sa.submap_align_session(p, pools, pairs, io, registration=reg, gt_poses=gt if any(g is not None for g in gt) else None)
    assert list(got) == blocks
    return got, want, ctx2, blocks


CASES = [dict(name="one-robot", R=1, empty=(), pairs=None, desc=None, gt=(), fill=()),
         dict(name="three-robots-one-empty-gt-on-one", R=3, empty=(1,), pairs=None, desc='mean_semantic', gt=(0,), fill=()),
         dict(name="off-diagonal-only-gt-on-all", R=3, empty=(), pairs=[(2, 0), (0, 1)], desc=None, gt=(0, 1, 2), fill=()),
         dict(name="fill-and-radius-pools-descriptor", R=3, empty=(), pairs=None, desc='mean_semantic', gt=(), fill=(0, 2)),
         dict(name="fill-pools-no-descriptor", R=2, empty=(), pairs=None, desc=None, gt=(1,), fill=(0, 1))]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_session_equals_submap_align_pools_per_block_in_aabb_mode(case):
    R = case["R"]
    if R == 1:                                               # two laps of one map (tests/_self_pools.py): loops close between the laps
        p, io = sp.params_of(sp.CASES[0])
        p.submap_radius = None
        reg = p.get_object_registration()
        pools = [sp.build_pool(sp.CASES[0], reg, so.OracleSubmapContext(), "cpu")[0]]
    else:
        reg, pools = make_pools(case["desc"], R, case["empty"])
        for r in case["fill"]:
            pools[r] = fill_pool(reg, r, case["desc"])
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, force_fill_submaps=True, submap_descriptor=case["desc"],
                              submap_descriptor_thresh=0.8, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
        io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    gt = [gt_for(pools[r], 70 + r) if r in case["gt"] else None for r in range(R)]
    got, want, ctx, blocks = run_both(p, io, reg, pools, case["pairs"], gt)
    assert ctx.session_aabb_gates == 1 and ctx.session_gates == 0 and ctx.gates == 0 and ctx.aabb_gates == 0 and ctx.boxes == 0 and ctx.tails == 1
    assert ctx.order[:2] == ["session_boxes", "session_gate"] and ctx.order[-1] == "tail" and len(ctx.session_boxes) == 1
    assert ctx.order.count("reduce") == (1 if any(r == s for r, s in blocks) else 0)
    aligned = edges = 0
    near = []
    for key in blocks:
        sx.exact(got[key], want[key], stand_in_sim_terms=D)
        assert got[key].submap_align_params.single_robot_lc == (key[0] == key[1])
        assert tuple(got[key].submap_io.gt_available) == (gt[key[0]] is not None, gt[key[1]] is not None)
        aligned += int((want[key].clipper_num_associations >= 4).sum()); edges += len(want[key].lc_edges["pairs"])
        near.append(~np.isnan(want[key].robots_nearby_mat).reshape(-1))
    near = np.concatenate(near)
    assert aligned >= 2 and edges >= 1, "hardly a pair aligned: the comparison would show nothing"
    assert near.any() and (~near).any(), "every pair or no pair is nearby: the gate would show nothing"
    if case["desc"]:
        sims = np.concatenate([want[k].similarity_mat.reshape(-1) for k in blocks])
        assert (sims < 0.8).any() and (sims >= 0.8).any()


def test_two_views_of_a_robot_get_two_box_sets():
    """Partners of 1 and of an even number of submaps read robot 0's poses an odd and an even number of times: two views, the same
    pool rows, a box set each — and every block still equals submap_align_pools."""
    reg, pools = make_pools(None, 3)
    c = pools[0].centers
    pools[0] = dataclasses.replace(pools[0], centers=dataclasses.replace(c, pose_flu=np.stack([alternating_pose(T[:3, 3]) for T in c.pose_flu])))
    one = pools[1].count.copy(); one[pools[1].nonempty[1:]] = 0          # robot 1 keeps one submap
    pools[1] = dataclasses.replace(pools[1], count=one)
    n = [len(q.nonempty) for q in pools]
    assert n[1] == 1 and n[2] % 2 == 0 and n[2] >= 2, n
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=None, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    blocks = [(0, 1), (0, 2), (2, 0)]
    got, want, ctx, _ = run_both(p, io, reg, pools, blocks, [None] * 3)
    assert ctx.table_robots == 4, ctx.table_robots                        # robot 0 twice, robots 1 and 2 once
    row0, count, T, box = ctx.session_boxes[0]
    assert len(count) == 2 * n[0] + n[1] + n[2]
    assert np.array_equal(row0[:n[0]], row0[n[0]:2 * n[0]]) and np.array_equal(count[:n[0]], count[n[0]:2 * n[0]])     # the same rows, twice
    for key in blocks:
        sx.exact(got[key], want[key])


def test_a_dim_2_pool_is_refused_once_the_context_exists():
    reg2, pools2, _ = gg._pools("roman", None, dim=2)
    ctx = sx.SessionAabbStubContext(); ctx.dim = 2; reg2.set_context(ctx)
    with pytest.raises(ValueError, match="submap_align_pools") as e:
        sa.submap_align_session(SubmapAlignParams(method="roman", semantics_dim=D, dim=2, submap_radius=None), pools2, None, sa.SubmapAlignIO(), registration=reg2)
    assert "rows hold no z" in str(e.value) and ctx.session_boxes == [] and ctx.session_aabb_gates == 0


def test_a_context_without_the_new_calls_is_refused_once_it_exists():
    reg, pools = make_pools(None, 2)
    made = []

    class Old(ss.SessionStubContext):
        """A context of the library before roman_session_boxes_dev / roman_session_gate_aabb_dev."""
    ctx = Old(); reg.set_context(ctx)
    real = reg._context
    reg._context = lambda: (made.append(1), real())[1]
    with pytest.raises(ValueError, match="roman_session_gate_aabb_dev") as e:
        sa.submap_align_session(SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=True), pools, None, sa.SubmapAlignIO(), registration=reg)
    assert "submap_align_pools" in str(e.value) and "roman_session_boxes_dev" in str(e.value) and made and ctx.session_gates == 0


# ---------------------------------------------------------------------------------------------
# RansacReg
# ---------------------------------------------------------------------------------------------
def test_ransac_refusals_come_before_a_context_is_made():
    pools, _ = trl._build("ransac")
    p = SubmapAlignParams(method="ransac", ransac_iter=trl.ITER, submap_max_size=8, submap_radius=15.0)
    io = sa.SubmapAlignIO(lc_association_thresh=trl.THRESH)

    def refused(pl, reg, text):
        with pytest.raises(ValueError, match="submap_align_pools") as e:
            sa.submap_align_session(p, pl, None, io, registration=reg)
        assert text in str(e.value), str(e.value)
    ctx = sx.SessionAabbStubContext()
    _, flat, _ = gg._pools("roman", None, dim=2)
    refused(flat, trl._ransac_reg(ctx), "no z")
    refused([dataclasses.replace(pools[0], cap=_abi.ROMAN_RANSAC_MAX_OBJECTS + 1), pools[1]], trl._ransac_reg(ctx), str(_abi.ROMAN_RANSAC_MAX_OBJECTS))
    assert ctx.order == [] and ctx.ransacs == []
    reg = trl._ransac_reg()
    refused(pools, reg, "no context")
    assert reg._ctx is None
    old = ss.SessionStubContext()
    refused(pools, trl._ransac_reg(old), "roman_ransac_lc_batch_dev")
    assert old.session_gates == 0 and old.order == []


@pytest.mark.parametrize("aabb", [False, True], ids=["radius", "aabb"])
def test_ransac_session_equals_submap_align_pools_per_block(aabb, orc):
    """Two robots and a robot of two laps (a self block with shared segment ids): every block through ONE RANSAC call."""
    pools, _ = trl._build("ransac")
    self_pool, _ = trl._self_pool()
    pools = [pools[0], pools[1], self_pool]
    p = SubmapAlignParams(method="ransac", ransac_iter=trl.ITER, submap_max_size=8, submap_radius=None if aabb else 15.0, single_robot_lc_time_thresh=200.0)
    io = sa.SubmapAlignIO(lc_association_thresh=trl.THRESH)
    blocks = [(0, 1), (2, 2), (1, 0)]
    reg = trl._ransac_reg()
    got, want, ctx, _ = run_both(p, io, reg, pools, blocks, [None] * 3)
    B = sum(len(want[k].timing_list) for k in blocks)
    assert ctx.ransacs == [(B, 3, True)] and ctx.tails == 1 and ctx.order[-2:] == ["ransac", "tail"] and "batch" not in ctx.order
    assert ctx.order.count("reduce") == 1 and (ctx.order[0] == "session_boxes") == aabb
    for key in blocks:
        sx.exact(got[key], want[key])
    n = np.concatenate([want[k].clipper_num_associations.reshape(-1) for k in blocks])
    assert (n >= trl.THRESH).sum() >= 2 and sum(len(want[k].lc_edges["pairs"]) for k in blocks) >= 1
    assert sum(len(want[k].timing_list) for k in blocks if k[0] != k[1]) >= 2 and len(want[(2, 2)].timing_list) >= 1


# ---------------------------------------------------------------------------------------------
# stacked frame descriptors behind the bounding-box gate, over force-fill pools
# ---------------------------------------------------------------------------------------------
def test_stacked_descriptors_over_force_fill_pools_on_a_stand_in(monkeypatch):
    """The 'fill-stacked' case of tests/test_gpu_submap_align_session_aabb.py — its pools, its conditions, its exact comparison —
    over the stand-in: the session's stacked similarity in front of session_gate_aabb_dev(sim_in) against stacked_sim_dev +
    grid_gate_aabb_dev(sim_in) per block (one oracle on both sides: the similarity bit for bit)."""
    import _frame_desc_oracle as fdo
    import test_gpu_submap_align_session_aabb as e2e

    class FillFrameContext(fdo.FrameCallsMixin, fo.OracleFillContext):
        """submaps_fill_dev and frame_select_dev through the oracles (build_submap_pool(fill=..., frames=...) on the host)."""
    ctx = sx.SessionAabbStackedStubContext()
    pools_, session_ = sa.submap_align_pools, sa.submap_align_session

    def per_pair(p, pl, *a, **k):                            # (the stand-in's batch call reads n_objects rows)
        ctx.n_objects = int(pl[0].pool.shape[0] + (0 if pl[0] is pl[1] else pl[1].pool.shape[0]))
        return pools_(p, pl, *a, **k)

    def session(p, pl, *a, **k):
        ctx.n_objects = int(sum(q.pool.shape[0] for q in pl)); ctx.order.clear()
        out = session_(p, pl, *a, **k)
        assert ctx.order[:3] == ["session_boxes", "session_stacked_sim", "session_gate"] and ctx.session_aabb_gates == 1 and len(ctx.session_boxes) == 1
        return out
    monkeypatch.setattr(sa, "submap_align_pools", per_pair); monkeypatch.setattr(sa, "submap_align_session", session)
    e2e.run_case("fill-stacked", ctx, "cpu", fill_ctx=FillFrameContext())
    assert ctx.aabb_gates == 6 and ctx.boxes == 12 and ctx.session_stacked_sims == 1
