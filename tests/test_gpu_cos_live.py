"""k_cos_live — the cosine stage, the single scores and the ordered live pools of a batch of all-to-all problems in one kernel per problem
(k_cos_sel's bf16 screen and exact f64 candidates, then k_live's gate, single_score() and ordered compaction in the same workgroup).
What must hold, against the dense kernels (ROMAN_COS_SEL=0: k_cos_deal's whole matrix, then k_live<0> / k_live<1>):
  * the live list of a problem — index and score of every live association, ascending — bit for bit (roman_debug_live);
  * every output of a batched call bit for bit: status, associations incl. order, poses, live counts, nnz, pass counts, scores;
  * also when some problems of the batch overflow the candidate list (they go to k_cos_deal + k_live, the rest through k_cos_live, in one
    call), for descriptor lengths that are not a multiple of the tile / chunk, and for pairs planted right at the gate
    (exact cosines in [cosine_min - 2^-7, cosine_min + 2^-7], the width of the screen's bound around the gate — but the planted descriptors
    are random, so their rounding errors cancel and the screen is off by ~2^-8 / sqrt(d) only; pairs whose rounding is the worst case, and
    the comparison with a plain exact cosine, are in tests/test_gpu_cos_screen_adversarial.py)."""
import numpy as np
import pytest

from conftest import registration_for
from roman_amd import synth
from roman_amd.align import batch as rb

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -7


def _pairs(rng, B, nlo, nhi, d, seed):
    pairs = []
    for k in range(B):
        n, m = int(rng.integers(nlo, nhi + 1)), int(rng.integers(nlo, nhi + 1))
        pr = synth.make_pair(n, m, d, 7000 + 10 * seed + k, tilt_deg=1.0)
        pairs.append((pr.map1, pr.map2))
    return pairs


def _plant_at_gate(rng, feats, lo, d, r1, r2, c):
    """Descriptor of row r2 := one whose exact cosine with row r1's is c (to rounding)."""
    a = feats[r1, lo:lo + d]
    u = a / np.linalg.norm(a)
    v = rng.standard_normal(d)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    feats[r2, lo:lo + d] = rng.uniform(0.3, 3.0) * (c * u + np.sqrt(1.0 - c * c) * v)


def _plant_batch(rng, reg, batch, per_problem=24):
    P = reg._abi_params()
    lo, d = P.point_dim + P.ratio_feature_dim, P.cos_feature_dim
    for b in range(len(batch.n1)):
        k = min(per_problem, int(batch.n1[b]), int(batch.n2[b]))
        for t in range(k):                       # pairs (t, t): distinct rows of both maps; half just above the gate, half just below
            c = P.cosine_min + (1 if t % 2 == 0 else -1) * rng.uniform(0.0, BOUND)
            _plant_at_gate(rng, batch.feats, lo, d, int(batch.off1[b]) + t, int(batch.off2[b]) + t, c)


def _both(monkeypatch, reg, batch):
    got = {}
    for setting in ("0", "0", "1"):              # (the first call of a parameter block sizes its workspace without a history)
        monkeypatch.setenv("ROMAN_COS_SEL", setting)
        got[setting] = rb.run_batch(reg, batch)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    return got["0"], got["1"]


def _same(a, b_, loose=()):
    """Every output bit for bit; for the problems in `loose` the solver's final score and step to 1e-12 (see the overflow test)."""
    assert np.array_equal(a.status, b_.status)
    for k in range(len(a.assoc)):
        assert np.array_equal(a.assoc[k], b_.assoc[k]), k
    assert np.array_equal(a.T, b_.T, equal_nan=True)
    exact = np.ones(len(a.status), dtype=bool); exact[list(loose)] = False
    for f in ("n_live", "nnz_upper", "n_pass", "outer_iters", "inner_iters", "ls_trials"):
        assert np.array_equal(a.stats[f], b_.stats[f]), f
    for f in ("score", "d_final"):
        assert np.array_equal(a.stats[f][exact], b_.stats[f][exact]), f
        assert np.allclose(a.stats[f][~exact], b_.stats[f][~exact], rtol=1e-12, atol=0.0), f


def _live(ctx, monkeypatch, P, D1, D2, setting):
    monkeypatch.setenv("ROMAN_COS_SEL", setting)
    ctx.score(P, D1, D2)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    return ctx.live()


@pytest.mark.parametrize("n1,n2,d,plant", [(200, 200, 512, False), (200, 200, 512, True), (37, 53, 70, True), (113, 97, 200, False),
                                           (256, 160, 64, True), (16, 16, 32, False), (90, 70, 15, True)])
def test_live_list_equals_the_dense_kernels_bit_for_bit(ctx, monkeypatch, n1, n2, d, plant):
    reg = registration_for("semanticgrav", semantics_dim=d); reg.set_context(ctx)
    P = reg._abi_params()
    pr = synth.make_pair(n1, n2, d, 500 + n1 + 3 * n2 + d, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    if plant:
        rng = np.random.default_rng(n1 + n2 + d)
        lo = P.point_dim + P.ratio_feature_dim
        F = np.vstack([D1, D2])
        for t in range(min(24, n1, n2)):
            c = P.cosine_min + (1 if t % 2 == 0 else -1) * rng.uniform(0.0, BOUND)
            _plant_at_gate(rng, F, lo, d, t, n1 + t, c)
        D2 = F[n1:].copy()
    idx0, sc0 = _live(ctx, monkeypatch, P, D1, D2, "0")
    idx1, sc1 = _live(ctx, monkeypatch, P, D1, D2, "1")
    assert len(idx0) > 0
    assert np.all(np.diff(idx1) > 0)
    assert np.array_equal(idx0, idx1)
    assert np.array_equal(sc0.view(np.uint64), sc1.view(np.uint64))
    if plant:                                    # the planted pairs above the gate are live, those below are not
        t = np.arange(min(24, n1, n2))
        planted = t * n2 + t
        assert np.isin(planted[t % 2 == 0], idx0).all() and not np.isin(planted[t % 2 == 1], idx0).any()


@pytest.mark.parametrize("B,nlo,nhi,d,seed,plant", [(24, 200, 200, 512, 1, False), (40, 30, 90, 33, 2, False), (9, 100, 140, 128, 3, False),
                                                    (16, 150, 200, 200, 4, True), (12, 60, 120, 77, 5, True)])
def test_a_batch_through_the_fused_kernel_equals_the_dense_kernels_bit_for_bit(ctx, monkeypatch, B, nlo, nhi, d, seed, plant):
    reg = registration_for("semanticgrav", semantics_dim=d); reg.set_context(ctx)
    rng = np.random.default_rng(seed)
    batch = rb.batch_from_pairs(reg, _pairs(rng, B, nlo, nhi, d, seed))
    assert batch.assoc is None                   # all-to-all: the fused kernel's batches
    if plant:
        _plant_batch(rng, reg, batch)
    a, b_ = _both(monkeypatch, reg, batch)
    assert (a.stats["n_live"] > 0).all()
    _same(a, b_)


def test_a_batch_in_which_some_problems_overflow_the_candidate_list(ctx, monkeypatch):
    """Problems whose descriptors are all alike (every cosine ~1: more candidates than the list holds) go to k_cos_deal + k_live, the rest
    of the batch through k_cos_live, in one call: every output as through the dense kernels.  (The two dense problems have ~4 500 live
    associations each and take the fallback solver, whose final score and step are sums in arrival order: those two to 1e-12.)"""
    d = 64
    reg = registration_for("semanticgrav", semantics_dim=d); reg.set_context(ctx)
    rng = np.random.default_rng(11)
    B = 10
    batch = rb.batch_from_pairs(reg, _pairs(rng, B, 60, 75, d, 11))
    P = reg._abi_params(); lo = P.point_dim + P.ratio_feature_dim
    for b in (2, 7):
        for off, n in ((batch.off1[b], batch.n1[b]), (batch.off2[b], batch.n2[b])):
            batch.feats[off:off + n, lo:lo + d] = 1.0 + 0.01 * rng.standard_normal((int(n), d))
    assert all(int(batch.n1[b]) * int(batch.n2[b]) > 4096 for b in (2, 7))
    a, b_ = _both(monkeypatch, reg, batch)
    ctx.sync()
    assert ctx.cosine_screen_stats()[2] == 2 / B            # the two problems went to the dense kernels, the others did not
    assert (a.stats["n_live"] > 0).all()
    _same(a, b_, loose=(2, 7))
