"""submap_align_pools / submap_align_session with num_solutions=K over a stand-in context (tests/_mno_lc.stub_context: the gate and
the shared-segment removal of the neighbouring CPU tests, the K solves through the oracle's mno loop, the tail through the host
statement) against a per-pair loop: the oracle's mno_clipper on the pair's segments, the host tail with the inputs the gate wrote,
the best rule; and the refusals that need no context, with a registration whose _context() raises."""
import copy

import numpy as np
import pytest

import _mno_lc as ml
import _session as ss
import _submaps_oracle as so
from _mno_oracle import oracle_mno, pose_of
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.ransac_reg import RansacReg
from test_grid_gate_cpu import D, _pools

THRESH = 4


def _setup(method, aabb=False, descriptor=None):
    reg, pools, segs = _pools(method, descriptor)
    ctx = ml.stub_context(); ctx.n_objects = int(pools[0].pool.shape[0] + pools[1].pool.shape[0]); reg.set_context(ctx)
    kw = dict(force_fill_submaps=True) if aabb else {}
    p = SubmapAlignParams(method=method, semantics_dim=D, submap_radius=15.0, submap_descriptor=descriptor,
                          submap_descriptor_thresh=0.8 if descriptor else 0.0, **kw)
    return reg, pools, segs, ctx, p, sa.SubmapAlignIO(lc_association_thresh=THRESH)


def _per_pair_loop(orc, reg, subs, lc, K):
    """The expectation: per registered pair (lc.iL, lc.iR) the oracle's mno_clipper, poses, the host tail, the best rule."""
    B = len(lc.iL)
    T = np.full((B, K, 4, 4), np.nan); n = np.zeros((B, K), np.int32); st = np.zeros((B, K), np.int32); assoc = []
    for b, (i, j) in enumerate(zip(lc.iL, lc.iR)):
        m1, m2 = subs[0][i].segments, subs[1][j].segments
        sols = oracle_mno(orc, reg, m1, m2, K)
        assoc.append([s["assoc"] for s in sols])
        for k, s in enumerate(sols):
            n[b, k] = len(s["assoc"])
            if n[b, k] >= 3:
                T[b, k] = pose_of(orc, m1, m2, s["assoc"])
            else:
                st[b, k] = _abi.ROMAN_ST_INSUFFICIENT
    rec, best, acc, acc_best = ml.mno_lc_tail(lc, K, T, n, st)
    return rec.reshape(B, K), best, acc_best, assoc


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("gate", ["radius", "aabb"])
def test_pools_equal_the_per_pair_loop(orc, K, gate):
    reg, pools, segs, ctx, p, io = _setup("gravity", aabb=(gate == "aabb"))
    got = sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=K)
    assert ctx.order.count("mno_tail") == 1 and "mno" in ctx.order and "batch" not in ctx.order and "tail" not in ctx.order
    lc = ctx.mno_tail_inputs[0]
    subs = [q.to_submaps(s) for q, s in zip(pools, segs)]
    rec, best, acc_best, assoc = _per_pair_loop(orc, reg, subs, lc, K)
    B = len(best)
    assert B > 3 and len(got.hypotheses) == B
    assert len(acc_best) >= 1 and len(acc_best) < B, "the comparison needs an accepted pair and one that is not"
    for b, (i, j) in enumerate(zip(lc.iL.tolist(), lc.iR.tolist())):
        r = rec[b, max(best[b], 0)]
        assert got.clipper_num_associations[i, j] == r["n_assoc"]
        np.testing.assert_allclose(got.T_ij_hat_mat[i, j], r["T_hat"], rtol=0, atol=1e-12, equal_nan=True)
        want_objs = assoc[b][best[b]] if best[b] >= 0 else np.zeros((0, 2))
        assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want_objs).reshape(-1, 2))
        hyps = got.hypotheses[(i, j)]
        assert len(hyps) == K
        for k, (a, score, T_hat, n, flags, edge) in enumerate(hyps):
            assert np.array_equal(a, assoc[b][k]) and n == rec[b, k]["n_assoc"] and flags == rec[b, k]["flags"]
            assert (edge is not None) == bool(flags & _abi.ROMAN_LC_ACCEPTED)
            if edge is not None:
                np.testing.assert_allclose(edge[0], rec[b, k]["edge_t"], atol=1e-12); np.testing.assert_allclose(edge[1], rec[b, k]["edge_q"], atol=1e-12)
    want_pairs = np.stack([lc.iL[acc_best], lc.iR[acc_best]], axis=1)
    assert np.array_equal(got.lc_edges["pairs"], want_pairs)
    np.testing.assert_allclose(got.lc_edges["t"], np.array([rec[b, best[b]]["edge_t"] for b in acc_best]), atol=1e-12)


def test_skipped_problems_are_issued_again_before_the_tail(orc):
    reg, pools, segs, ctx, p, io = _setup("gravity")
    want = sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=2)
    ctx2 = ml.stub_context(); ctx2.n_objects = ctx.n_objects; reg.set_context(ctx2)
    batch, _ = pools[0].grid_batch(pools[1], mask=~np.isnan(want.clipper_num_associations))
    ctx2.mno_skip_once = {(int(batch.off1[1]), int(batch.off2[1])), (int(batch.off1[2]), int(batch.off2[2]))}
    got = sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=2)
    assert len(ctx2.mno_calls) == len(ctx.mno_calls) + 1 and ctx2.mno_calls[-1] == 2     # the two skipped problems, once more, in one run
    assert np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])


def test_self_block_and_session_with_an_empty_robot(orc):
    """[pool, pool] self loop closures (associations index the reduced lists) and a session of three robots, one of them empty:
    every block equals submap_align_pools(num_solutions=2) for that block alone."""
    import _self_pools as sp
    case = dict(method="gravity", descriptor=None, thresh=0.0)
    reg = SubmapAlignParams(method="gravity", semantics_dim=D).get_object_registration()
    import dataclasses
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p, io = sp.params_of(case)
    p = dataclasses.replace(p, submap_max_size=10)           # (10 x 10 associations a pair: the oracle's dense solves stay at milliseconds)
    params = SubmapParams.from_submap_align_params(p)
    laps = sp.two_lap_map(n_lap=100)
    build = lambda sg, traj, times: build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params,
                                                      ctx=so.OracleSubmapContext(), device="cpu")
    pool = build(*laps)
    sg, traj, times = ss.robot_view(*laps, 1, keep=0.85, last_pose=sp.N_POSES)
    other, empty = build(sg, traj, times), build(sg, traj[:0], times[:0])
    pools = [pool, other, empty]
    blocks = [(0, 0), (0, 1), (1, 2), (2, 2)]
    want = {}
    for r, s in blocks:
        ctx = ml.stub_context(); reg.set_context(ctx); ctx.n_objects = 0
        q = copy.copy(p); q.single_robot_lc = (r == s)
        want[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg, num_solutions=2)
        if (r, s) == (0, 0):
            assert "reduce" in ctx.order and len(want[(r, s)].lc_edges["pairs"]) >= 1
    ctx = ml.stub_context(); reg.set_context(ctx); ctx.n_objects = 0
    got = sa.submap_align_session(p, pools, blocks, io, registration=reg, num_solutions=2)
    assert ctx.order.count("mno_tail") == 1
    for blk in blocks:
        ss.compare(got[blk], want[blk])
        assert set(got[blk].hypotheses) == set(want[blk].hypotheses)
        for key, hyps in want[blk].hypotheses.items():
            for a, b in zip(got[blk].hypotheses[key], hyps):
                assert np.array_equal(a[0], b[0]) and a[3:5] == b[3:5] and (a[5] is None) == (b[5] is None)
    assert got[(1, 2)].hypotheses == {} and got[(2, 2)].hypotheses == {}


class _NoContext:
    """A registration whose _context() raises: every refusal below comes before a context is made."""

    def __init__(self, reg):
        self.__dict__["_reg"] = reg

    def __getattr__(self, name):
        if name == "_context":
            raise AssertionError("a context was asked for before the refusal")
        return getattr(self._reg, name)


@pytest.mark.parametrize("fn", ["pools", "session"])
def test_refusals_before_a_context(fn):
    reg, pools, segs, ctx, p, io = _setup("gravity")
    call = (lambda r, K, pl=pools: sa.submap_align_pools(p, pl, io, registration=r, num_solutions=K)) if fn == "pools" else \
           (lambda r, K, pl=pools: sa.submap_align_session(p, pl, None, io, registration=r, num_solutions=K))

    class Ransac(RansacReg):
        def _context(self):
            raise AssertionError("a context was asked for before the refusal")
    with pytest.raises(ValueError, match="RansacReg builds no affinity matrix"):
        call(Ransac(3), 2)
    none = _NoContext(reg)
    for K in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_solutions must be an integer in 1 ... 64"):
            call(none, K)
    big = [copy.copy(q) for q in pools]
    for q in big:
        q.cap = 56                                           # 56 * 56 = 3136 > ROMAN_MNO_MAX_ASSOC
    with pytest.raises(ValueError, match="ROMAN_MNO_MAX_ASSOC"):
        call(none, 2, big)


def test_a_context_without_the_tail_is_refused():
    reg, pools, segs, ctx, p, io = _setup("gravity")
    import _session_aabb as sab
    old = sab.SessionAabbStubContext(); old.n_objects = ctx.n_objects; reg.set_context(old)
    with pytest.raises(ValueError, match="the context has no roman_mno_lc_tail_dev"):
        sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=2)
    with pytest.raises(ValueError, match="the context has no roman_mno_lc_tail_dev"):
        sa.submap_align_session(p, pools, None, io, registration=reg, num_solutions=2)


def test_none_takes_the_single_solution_path():
    reg, pools, segs, ctx, p, io = _setup("gravity")
    res = sa.submap_align_pools(p, pools, io, registration=reg)
    assert "mno" not in ctx.order and "batch" in ctx.order and ctx.order[-1] == "tail" and res.hypotheses is None
