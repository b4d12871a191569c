"""Self loop closures on the device-resident pools path without a GPU: the reduced-problem arithmetic behind
roman_shared_reduce_dev on hand-made counts, submap_align_pools(p, [pool, pool]) over stand-in contexts against submap_align_grid
with the CPU double for `compute` — the fixture and the conditions of tests/test_gpu_self_pools.py —, the path pools without shared
ids keep, and the refusal that stays."""
import dataclasses

import numpy as np
import pytest

import _lc_tail
import _self_pools as sp
import _submaps_oracle as so
from roman_amd import _abi
from roman_amd.align import submap_align as sa
from test_grid_gate_cpu import PoolsStubContext


class SelfPoolsStubContext(PoolsStubContext):
    """PoolsStubContext plus roman_shared_reduce_dev through the NumPy model; the batch call then reads pool + region."""

    def __init__(self, dim=3):
        super().__init__(0, dim)
        self.reduces = []

    def shared_reduce_dev(self, B, F, feats_ptr, region_row0, ids_ptr, off1, n1, off2, n2, keep_ptr, kept_ptr):
        self.order.append("reduce")
        self.reduces.append((int(B), int(region_row0)))
        sp.shared_reduce_model(B, F, feats_ptr, region_row0, ids_ptr, off1, n1, off2, n2, keep_ptr, kept_ptr)
        self.n_objects = int(region_row0) + int(np.sum(n1, dtype=np.int64) + np.sum(n2, dtype=np.int64))


def test_reduced_problems_on_hand_made_counts():
    off1 = np.array([0, 40, 0, 80, 7], dtype=np.int64); n1 = np.array([3, 5, 3, 0, 2], dtype=np.int32)
    off2 = np.array([40, 0, 0, 90, 9], dtype=np.int64); n2 = np.array([5, 3, 3, 4, 6], dtype=np.int32)
    kept = np.array([[3, 5],        # nothing lost: as given
                     [4, 3],        # side 1 lost one
                     [0, 0],        # the same submap on both sides: both empty
                     [0, 4],        # an empty side that lost nothing: as given
                     [2, 1]],       # side 2 lost five
                    dtype=np.int32)
    o1, m1, o2, m2 = sa.reduced_problems(off1, n1, off2, n2, kept, 1000)
    kb = np.array([0, 8, 16, 22, 26])
    assert o1.tolist() == [0, 1000 + 8, 1000 + 16, 80, 1000 + 26] and m1.tolist() == [3, 4, 0, 0, 2]
    assert o2.tolist() == [40, 1000 + 8 + 5, 1000 + 16 + 3, 90, 1000 + 26 + 2] and m2.tolist() == [5, 3, 0, 4, 1]
    assert o1.dtype == o2.dtype == np.int64 and m1.dtype == m2.dtype == np.int32
    assert np.all(o1[[1, 2, 4]] == 1000 + kb[[1, 2, 4]])
    e64, e32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    assert all(len(x) == 0 for x in sa.reduced_problems(e64, e32, e64, e32, np.zeros((0, 2), np.int32), 5))
    # offsets past 2^31 stay exact
    big = sa.reduced_problems(off1, n1, off2, n2, kept, 2 ** 33)
    assert big[0][4] == 2 ** 33 + 26 and big[2][4] == 2 ** 33 + 28
    for bad in (np.array([[4, 5]] + kept[1:].tolist()), np.array([[3, -1]] + kept[1:].tolist()), kept[:4]):
        with pytest.raises(_abi.RomanHipError):
            sa.reduced_problems(off1, n1, off2, n2, bad, 1000)


@pytest.fixture(scope="module", params=sp.CASES, ids=[c["name"] for c in sp.CASES])
def stand_in_run(request):
    case = request.param
    ctx = SelfPoolsStubContext()
    got, want, pool = sp.run_case(case, ctx, "cpu", build_ctx=so.OracleSubmapContext(), compute=_lc_tail.oracle_lc_compute)
    return case, ctx, got, want, pool


def test_self_pools_equal_the_grid_path_on_a_stand_in(stand_in_run):
    case, ctx, got, want, pool = stand_in_run
    print(sp.conditions(case, want, pool))
    sp.compare(got, want)
    assert ctx.order[0] == "gate" and ctx.order[1] == "reduce" and ctx.order[-1] == "tail" and ctx.order.count("reduce") == 1
    assert ctx.reduces[0] == (len(got.timing_list), int(pool.pool.shape[0]))      # every registered pair, the region behind the pool's rows
    assert pool.ids_dev is not None and np.array_equal(pool.ids_dev.numpy(), pool.ids.reshape(-1))


def test_pools_without_shared_ids_take_the_old_path():
    from test_grid_gate_cpu import _pools
    reg, pools, segs = _pools("roman", None)                 # the second map has its own ids
    from roman_amd.align import SubmapAlignParams
    p = SubmapAlignParams(method="roman", semantics_dim=16, submap_radius=15.0, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    ctx = SelfPoolsStubContext()
    ctx.n_objects = int(pools[0].pool.shape[0] + pools[1].pool.shape[0])
    reg.set_context(ctx)
    sa.submap_align_pools(p, pools, sa.SubmapAlignIO(lc_association_thresh=4), registration=reg)
    assert ctx.reduces == [] and "reduce" not in ctx.order and ctx.gates == 1 and ctx.tails == 1


def test_shared_ids_over_a_pool_without_ids_dev_are_refused():
    case = sp.CASES[1]
    p, io = sp.params_of(case)
    reg = p.get_object_registration()
    ctx = SelfPoolsStubContext(); reg.set_context(ctx)
    pool, _ = sp.build_pool(case, reg, so.OracleSubmapContext(), "cpu")
    bare = dataclasses.replace(pool, ids_dev=None)           # a pool built by other means
    with pytest.raises(ValueError, match="to_submaps") as e:
        sa.submap_align_pools(p, [bare, bare], io, registration=reg)
    assert "ids_dev" in str(e.value) and "submap_align_grid" in str(e.value) and ctx.gates == 0
