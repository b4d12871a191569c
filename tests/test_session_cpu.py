"""A whole session in one call without a GPU: the NumPy oracle of the session gate against pass 1 of
submap_align_grid per block, and submap_align_session over a stand-in context against submap_align_pools called per block on the
same pools with the same stand-in."""
import copy
import dataclasses

import numpy as np
import pytest

import _grid_gate_oracle as go
import _lc_tail
import _self_pools as sp
import _session as ss
import _submaps_oracle as so
from roman_amd import synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.runtime import session_tables
from test_grid_gate_cpu import _failing_compute, _submaps_of, close

D = 16


# ---------------------------------------------------------------------------------------------
# the oracle: per block it is tests/_grid_gate_oracle.py, which test_grid_gate_cpu.py checks against submap_align_grid; here the
# slicing, the ground-truth rule per block and the global indices are checked the same way
# ---------------------------------------------------------------------------------------------
def test_session_tables_match_the_written_out_prefixes():
    counts = [5, 0, 6, 3]
    blocks = [(0, 0, True), (0, 2, False), (1, 2, False), (3, 2, False), (2, 2, True)]
    for got, want in zip(session_tables(counts, blocks), ss.tables(counts, blocks)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert ss.tables(counts, blocks)[3].tolist() == [0, 10, 20, 20, 26, 38]          # 5 * 2, 5 * 2, 0, 3 * 2, 6 * 2


@pytest.mark.parametrize("d,has_gt", [(0, (0, 0, 0)), (16, (1, 0, 1)), (7, (1, 1, 1))])
def test_oracle_equals_pass_1_of_submap_align_grid_per_block(d, has_gt):
    counts = [5, 3, 6]
    gate = dict(radius=12.0, skip_distance=40.0, desc_thresh=0.6 if d else 0.0, lc_time_thresh=60.0)
    rng = np.random.default_rng(900 + d)
    sides = [go.random_side(rng, n, max(d, 1), with_gt=True) for n in counts]
    blocks = [(0, 0, True), (0, 1, False), (0, 2, False), (1, 1, True), (2, 1, False), (2, 2, True)]
    for r0, r1, lc in blocks:
        assert not go.borderline(sides[r0], sides[r1], single_robot_lc=lc, **gate), "choose another seed"
    subs = [_submaps_of(s, rng, d > 0) for s in sides]
    for r, (side, sms) in enumerate(zip(sides, subs)):       # the sides as the caller resolves them
        if not has_gt[r]:
            for sm in sms:
                sm.pose_flu_gt = None
        side["T_w"] = np.stack([sa.transform_rm_roll_pitch(np.array(sm.pose_flu_gt if has_gt[r] else sm.pose_flu)) for sm in sms])
    arr = {k: np.concatenate([s[k] for s in sides]) for k in ("pos", "pos_gt", "T_w", "time")}
    arr["desc"] = np.concatenate([s["desc"] for s in sides]) if d else None
    sub_off, blk, pair_off, _ = ss.tables(counts, blocks)
    o = ss.session_gate_oracle(arr, sub_off, blk, has_gt, **gate)
    assert o["todo_off"][-1] == len(o["pairs"]) and o["dist"].shape == (pair_off[-1],)
    for b, (r0, r1, lc) in enumerate(blocks):
        p = SubmapAlignParams(submap_radius=gate["radius"], submap_descriptor='mean_semantic' if d else None, submap_descriptor_thresh=gate["desc_thresh"],
                              single_robot_lc=False)
        io = sa.SubmapAlignIO(skip_distance=gate["skip_distance"], gt_available=(bool(has_gt[r0]), bool(has_gt[r1])))
        seen = []
        res = sa.submap_align_grid(p, [copy.deepcopy(subs[r0]), copy.deepcopy(subs[r1])], io, registration=_lc_tail.StubRegistration(3, False),
                                   compute=_failing_compute(seen))
        n0, n1 = counts[r0], counts[r1]
        lo, hi = pair_off[b], pair_off[b + 1]
        flags = o["flags"][lo:hi].reshape(n0, n1)
        nearby = (flags & go.NEARBY) != 0
        assert np.array_equal(np.where(nearby, o["dist"][lo:hi].reshape(n0, n1), np.nan), res.robots_nearby_mat, equal_nan=True)
        gp = o["pairs"][o["todo_off"][b]:o["todo_off"][b + 1]].astype(np.int64)
        assert np.array_equal(gp - [sub_off[r0], sub_off[r1]], seen[0] if seen else np.zeros((0, 2)))
        assert close(o["T_ij"][lo:hi].reshape(n0, n1, 4, 4), res.T_ij_mat) and close(o["yaw_deg"][lo:hi].reshape(n0, n1), res.submap_yaw_diff_mat)
        dt = np.abs(arr["time"][gp[:, 0]] - arr["time"][gp[:, 1]])
        assert np.array_equal(o["enable"][o["todo_off"][b]:o["todo_off"][b + 1]], np.where(lc & (dt < 60.0), 0, 1))
        assert np.array_equal(o["T_ref"][o["todo_off"][b]:o["todo_off"][b + 1]], o["T_ij"][lo:hi][(gp[:, 0] - sub_off[r0]) * n1 + gp[:, 1] - sub_off[r1]])
    self_enable = np.concatenate([o["enable"][o["todo_off"][b]:o["todo_off"][b + 1]] for b, x in enumerate(blocks) if x[2]])
    assert 0 < self_enable.sum() < len(self_enable)


# ---------------------------------------------------------------------------------------------
# submap_align_session over the stand-in against submap_align_pools per block
# ---------------------------------------------------------------------------------------------
VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None, max_size=12), dict(keep=0.8, first_pose=3, last_pose=None, max_size=10),
         dict(keep=0.9, first_pose=0, last_pose=19, max_size=14)]


def make_pools(descriptor, n_robots, empty=()):
    """`n_robots` maps of the same place (cross pairs hold true matches), every robot with its OWN view of it (tests/_session.
    robot_view: other segments, other centres, another stretch of the drive) and its own pool shape (other cap): no two pools
    have the same rows, row count or number of submaps, so a problem that read another robot's rows would show.  A robot in
    `empty` drives where no segment is: its pool has centres and no non-empty submap."""
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    base = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
    pools = []
    for r in range(n_robots):
        v = VIEWS[r]
        params = SubmapParams(max_size=v["max_size"], radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor=descriptor)
        sg, traj, times = ss.robot_view(*base, r, keep=v["keep"], first_pose=v["first_pose"], last_pose=v["last_pose"])
        if r in empty:
            for T in traj:
                T[:3, 3] += (5000.0, 0.0, 0.0)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=so.OracleSubmapContext(), device="cpu"))
    live = [q for r, q in enumerate(pools) if r not in empty]
    assert len({int(q.pool.shape[0]) for q in live}) == len(live) and len({int(q.cap) for q in live}) == len(live), "two robots have pools of one shape"
    return reg, pools


def gt_for(pool, seed):
    """Ground-truth poses of every centre: the odometry pose a little off (yaw-only, as the pools' poses are)."""
    rng = np.random.default_rng(seed)
    gt = np.array(pool.centers.pose_flu, dtype=np.float64).copy()
    gt[:, :3, 3] += rng.normal(0.0, 0.4, (len(gt), 3))
    return gt


def per_block(p, io, reg, pools, blocks, gt):
    out = {}
    ctx = reg._context()
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        bio = copy.copy(io); bio.gt_available = (gt[r] is not None, gt[s] is not None)
        ctx.n_objects = int(pools[r].pool.shape[0] + pools[s].pool.shape[0])
        out[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], bio, registration=reg, gt_poses=(gt[r], gt[s]))
    return out


CASES = [dict(name="one-robot", R=1, empty=(), pairs=None, desc='mean_semantic', gt=()),
         dict(name="three-robots-one-empty", R=3, empty=(1,), pairs=None, desc='mean_semantic', gt=(0,)),
         dict(name="off-diagonal-only", R=3, empty=(), pairs=[(2, 0), (0, 1)], desc=None, gt=(0, 1, 2)),
         dict(name="no-descriptor-all-pairs", R=2, empty=(), pairs=None, desc=None, gt=())]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_session_equals_submap_align_pools_per_block_on_a_stand_in(case):
    R = case["R"]
    if R == 1:                                               # two laps of one map (tests/_self_pools.py): loops close between the laps
        p, io = sp.params_of(sp.CASES[0])
        p.single_robot_lc = False                            # (ignored by the session call: the block's own rule holds)
        reg = p.get_object_registration()
        pools = [sp.build_pool(sp.CASES[0], reg, so.OracleSubmapContext(), "cpu")[0]]
    else:
        reg, pools = make_pools(case["desc"], R, case["empty"])
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor=case["desc"], submap_descriptor_thresh=0.8,
                              single_robot_lc=True, single_robot_lc_time_thresh=40.0)        # (single_robot_lc is ignored by the session call)
        io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    gt = [gt_for(pools[r], 70 + r) if r in case["gt"] else None for r in range(R)]
    blocks = case["pairs"] or [(r, s) for r in range(R) for s in range(r, R)]
    ctx = ss.SessionStubContext(); reg.set_context(ctx)
    want = per_block(p, io, reg, pools, blocks, gt)
    ctx2 = ss.SessionStubContext(); reg.set_context(ctx2)
    ctx2.n_objects = int(sum(q.pool.shape[0] for q in pools if len(q.nonempty)))
    got = sa.submap_align_session(p, pools, case["pairs"], io, registration=reg, gt_poses=gt if case["gt"] else None)
    assert list(got) == blocks
    assert ctx2.session_gates == 1 and ctx2.gates == 0 and ctx2.tails == 1 and ctx2.order[0] == "session_gate" and ctx2.order[-1] == "tail"
    assert ctx2.order.count("reduce") == (1 if any(r == s for r, s in blocks) else 0)
    aligned = edges = 0
    for key in blocks:
        ss.compare(got[key], want[key])
        assert got[key].submap_align_params.single_robot_lc == (key[0] == key[1])
        assert tuple(got[key].submap_io.gt_available) == (gt[key[0]] is not None, gt[key[1]] is not None)
        aligned += int((want[key].clipper_num_associations >= 4).sum()); edges += len(want[key].lc_edges["pairs"])
    assert aligned >= 2 and edges >= 1, "hardly a pair aligned: the comparison would show nothing"
    for r in case["empty"]:
        for key in blocks:
            if r in key:
                assert 0 in got[key].clipper_num_associations.shape and len(got[key].lc_edges["pairs"]) == 0


def alternating_pose(t):
    """A yaw-only pose at `t` whose flattening alternates between two neighbouring values (F(F(T)) != F(T), F(F(F(T))) == F(T)): the
    pose a pair loop leaves behind then depends on whether it read it an even or an odd number of times."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a = sa.transform_rm_roll_pitch(go.yaw_pose(rng.uniform(-np.pi, np.pi), t))
        b = sa.transform_rm_roll_pitch(a.copy()); c = sa.transform_rm_roll_pitch(b.copy()); e = sa.transform_rm_roll_pitch(c.copy())
        if b.tobytes() != c.tobytes() and e.tobytes() == b.tobytes():
            return a
    raise AssertionError("no alternating pose among 2000 yaws: the case cannot be built here")


def test_a_robot_whose_pose_depends_on_the_read_count_gets_one_view_per_outcome():
    """Partners of 1 and of several submaps read robot 0's poses an odd and an even number of times; where that gives two reference
    poses the robot enters the gate's tables twice, and every block still equals submap_align_pools."""
    reg, pools = make_pools(None, 3)
    c = pools[0].centers
    pools[0] = dataclasses.replace(pools[0], centers=dataclasses.replace(c, pose_flu=np.stack([alternating_pose(T[:3, 3]) for T in c.pose_flu])))
    one = pools[1].count.copy(); one[pools[1].nonempty[1:]] = 0          # robot 1 keeps one submap
    pools[1] = dataclasses.replace(pools[1], count=one)
    n = [len(q.nonempty) for q in pools]
    assert n[1] == 1 and n[2] % 2 == 0 and n[2] >= 2, n                   # an odd and an even number of reads of robot 0's poses
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    blocks = [(0, 1), (0, 2), (2, 0)]
    ctx = ss.SessionStubContext(); reg.set_context(ctx)
    want = per_block(p, io, reg, pools, blocks, [None] * 3)
    ctx2 = ss.SessionStubContext(); reg.set_context(ctx2)
    ctx2.n_objects = int(sum(q.pool.shape[0] for q in pools))
    got = sa.submap_align_session(p, pools, blocks, io, registration=reg)
    assert ctx2.table_robots == 4, ctx2.table_robots                      # robot 0 twice, robots 1 and 2 once
    for key in blocks:
        ss.compare(got[key], want[key])
        assert np.array_equal(got[key].T_ij_mat, want[key].T_ij_mat)


def test_a_session_without_pairs_makes_no_context():
    reg, pools = make_pools(None, 2, empty=(0, 1))
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    got = sa.submap_align_session(SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0), pools, None, sa.SubmapAlignIO(), registration=reg)
    assert list(got) == [(0, 0), (0, 1), (1, 1)] and all(r.clipper_num_associations.shape == (0, 0) for r in got.values())
    assert sa.submap_align_session(SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0), [], None, registration=reg) == {}


def test_session_refuses_what_it_does_not_cover_before_a_context_is_made():
    reg, pools = make_pools('mean_semantic', 2)
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    base = dict(method="roman", semantics_dim=D, submap_radius=15.0)
    io = sa.SubmapAlignIO()
    _, bare = make_pools(None, 2)
    other_len = dataclasses.replace(pools[1], desc_dev=pools[1].desc_dev[:, :8].contiguous())
    import torch
    wide = dataclasses.replace(pools[1], pool=torch.cat([pools[1].pool, pools[1].pool[:, :1]], dim=1))
    no_ids = dataclasses.replace(pools[0], ids_dev=None)
    ransac = SubmapAlignParams(method="ransac").get_object_registration()
    ransac._context = reg._context
    prune = SubmapAlignParams(method="clipper+prune", semantics_dim=D).get_object_registration()
    prune._context = reg._context
    cases = [
        (SubmapAlignParams(**base, force_fill_submaps=True), pools, None, reg, "bounding boxes"),
        (SubmapAlignParams(**{**base, "submap_radius": None}), pools, None, reg, "bounding boxes"),
        (SubmapAlignParams(**base, submap_descriptor='stacked_frame_descriptors'), pools, None, reg, "stacked_frame_descriptors"),
        (SubmapAlignParams(**base, submap_descriptor='mean_frame_descriptor'), pools, None, reg, "mean_frame_descriptor"),
        (SubmapAlignParams(**{**base, "method": "ransac"}), pools, None, ransac, "RansacReg"),
        (SubmapAlignParams(**{**base, "method": "clipper+prune"}), pools, None, prune, "prefilter"),
        (SubmapAlignParams(**base), [pools[0], wide], None, reg, "row widths"),
        (SubmapAlignParams(**base, submap_descriptor='mean_semantic'), [pools[0], other_len], None, reg, "different lengths"),
        (SubmapAlignParams(**base, submap_descriptor='mean_semantic'), bare, None, reg, "mean_semantic"),
        (SubmapAlignParams(**base), [no_ids, pools[1]], None, reg, "ids_dev"),
        (SubmapAlignParams(**base), pools, [(0, 2)], reg, "robot_pairs"),
        (SubmapAlignParams(**base), pools, [(0, 1), (0, 1)], reg, "robot_pairs"),
    ]
    for p, pl, pairs, r, what in cases:
        with pytest.raises(ValueError, match="submap_align_pools") as e:
            sa.submap_align_session(p, pl, pairs, io, registration=r)
        assert what in str(e.value), (what, str(e.value))
    with pytest.raises(ValueError, match="submap_align_pools"):
        sa.submap_align_session(SubmapAlignParams(**base), pools, None, io, registration=reg, gt_poses=[None])
    # a pool without ids serves a session that holds no self block of it
    no_ids_ok = SubmapAlignParams(**base)
    reg2, _ = make_pools(None, 1)
    ctx = ss.SessionStubContext(); ctx.n_objects = int(no_ids.pool.shape[0] + pools[1].pool.shape[0]); reg2.set_context(ctx)
    got = sa.submap_align_session(no_ids_ok, [no_ids, pools[1]], [(0, 1)], io, registration=reg2)
    assert ctx.session_gates == 1 and "reduce" not in ctx.order and list(got) == [(0, 1)]
