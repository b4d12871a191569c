"""roman_session_boxes_dev / roman_session_boxes on the device against roman_submap_boxes_dev on the SAME device:
for any submap the box is BITWISE what that call writes for the same rows and the same transform.  The session's submap table names
rows by offset and count: out of order, and twice with different transforms (two views of one robot), and from the middle of a slot
(rows that overlap another submap's)."""
import numpy as np
import pytest

import _grid_gate_oracle as go
from _hipmem import Hip
from test_gpu_fill_boxes import general_pose
from test_gpu_grid_gate import Guarded

pytestmark = pytest.mark.gpu

CAP = 70                                                     # a wave takes a full submap's rows in two steps
COUNT = np.array([0, 1, 2, 63, 64, 65, CAP], np.int32)
FILL = -7.25


def slot_boxes(ctx, hip, pool_ptr, F, count, T):
    """roman_submap_boxes_dev over slots of CAP rows starting at pool_ptr -> (S, 6)."""
    S = len(count)
    box = hip.upload(np.full((S, 6), FILL))
    ctx.submap_boxes_dev(S, F, CAP, pool_ptr, hip.upload(np.asarray(count, np.int32)), hip.upload(np.ascontiguousarray(T).reshape(S, 16)), box)
    ctx.sync()
    return hip.download(box, (S, 6), np.float64)


def make_table(ctx, hip, F, seed):
    """A slot pool (one spare row behind it) and a session table over it: the slots in a shuffled order with their own transform
    (view 1), the same rows in another order with other transforms (view 2), and every slot from its second row on (rows inside
    another submap's).  -> (pool, pool_ptr, row0, count, T, want): `want` from three roman_submap_boxes_dev calls."""
    rng = np.random.default_rng(seed)
    S = len(COUNT)
    pool = rng.uniform(-40.0, 40.0, (S * CAP + 1, F))        # rows beyond a count hold values that would move the box
    pool_ptr = hip.upload(pool)
    poses = lambda: np.array([go.yaw_pose(rng.uniform(-np.pi, np.pi), rng.uniform(-30, 30, 3)) if k % 2 else general_pose(rng) for k in range(S)])
    T1, T2, T3 = poses(), poses(), poses()
    inner = np.maximum(COUNT - 1, 0).astype(np.int32)
    ref1, ref2 = slot_boxes(ctx, hip, pool_ptr, F, COUNT, T1), slot_boxes(ctx, hip, pool_ptr, F, COUNT, T2)
    ref3 = slot_boxes(ctx, hip, pool_ptr + 8 * F, F, inner, T3)             # the slots moved on by one row
    o1, o2, o3 = rng.permutation(S), rng.permutation(S), rng.permutation(S)
    row0 = np.concatenate([o1 * CAP, o2 * CAP, o3 * CAP + 1]).astype(np.int64)
    count = np.concatenate([COUNT[o1], COUNT[o2], inner[o3]]).astype(np.int32)
    T = np.concatenate([T1[o1], T2[o2], T3[o3]])
    want = np.concatenate([ref1[o1], ref2[o2], ref3[o3]])
    assert set(COUNT.tolist()) <= set(count.tolist()) and len(set(row0[:2 * S].tolist())) == S      # every count; view 2 names view 1's rows
    return pool, pool_ptr, row0, count, T, want


def run_dev(ctx, hip, S, F, pool_ptr, row0, count, T, shift=0):
    out = Guarded(hip, 6 * S, np.float64, FILL, shift)
    ctx.session_boxes_dev(S, F, pool_ptr, hip.upload(row0[:S]) if S else None, hip.upload(count[:S]) if S else None,
                          hip.upload(np.ascontiguousarray(T[:S]).reshape(-1)) if S else None, out.ptr)
    ctx.sync()
    return out.get().reshape(S, 6)                           # (get() asserts that nothing beyond the S rows was written)


@pytest.mark.parametrize("F", [3, 4, 775])
def test_boxes_equal_submap_boxes_dev_bitwise(ctx, F):
    hip = Hip()
    try:
        pool, pool_ptr, row0, count, T, want = make_table(ctx, hip, F, 100 + F)
        S = len(count)
        got = run_dev(ctx, hip, S, F, pool_ptr, row0, count, T)
        for g in range(S):
            assert got[g].tobytes() == want[g].tobytes(), (F, g, int(row0[g]), int(count[g]))
        empty = count == 0
        assert empty.any() and np.all(np.isposinf(got[empty, :3])) and np.all(np.isneginf(got[empty, 3:]))
        assert np.all(got[count == 1, :3] == got[count == 1, 3:])           # one row: a point
        again = run_dev(ctx, hip, S, F, pool_ptr, row0, count, T, shift=1)
        assert again.tobytes() == got.tobytes()                              # two runs, the output off its 16-byte boundary
        host = ctx.session_boxes(pool, row0, count, T)
        assert host.tobytes() == got.tobytes()
    finally:
        hip.free_all()


@pytest.mark.parametrize("S", [0, 1, 4, 5])
def test_table_lengths_around_a_workgroup_of_four_waves(ctx, S):
    """S = 4 fills a workgroup, S = 5 opens a second one with one live wave; S = 0 writes nothing; rows beyond S stay untouched."""
    hip = Hip()
    try:
        F = 4
        pool, pool_ptr, row0, count, T, want = make_table(ctx, hip, F, 200)
        pick = np.argsort(-count, kind="stable")             # the long submaps first: every S > 0 holds rows
        row0, count, T, want = row0[pick], count[pick], T[pick], want[pick]
        out = Guarded(hip, 6 * (S + 2), np.float64, FILL)
        args = [hip.upload(row0[:S]), hip.upload(count[:S]), hip.upload(np.ascontiguousarray(T[:S]).reshape(-1))] if S else [None, None, None]
        ctx.session_boxes_dev(S, F, pool_ptr, *args, out.ptr)
        ctx.sync()
        got = out.get().reshape(S + 2, 6)
        assert got[:S].tobytes() == want[:S].tobytes() and np.all(got[S:] == FILL)
        assert ctx.session_boxes(pool, row0[:S], count[:S], T[:S]).tobytes() == want[:S].tobytes()
    finally:
        hip.free_all()
