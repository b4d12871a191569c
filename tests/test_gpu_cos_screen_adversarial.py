"""The bf16 cosine screen (k_cos_sel / k_cos_live: cos_sel_body) at its WORST case, against a plain model and a plain exact cosine.

tests/test_gpu_cos_sel.py and tests/test_gpu_cos_live.py plant pairs at the gate with random descriptors, whose rounding errors cancel
(the screen is then off by ~2^-8 / sqrt(d)), and compare with the dense HIP kernel.  Here the planted pairs come from
tests/_bf16_screen.py: every element beside a bf16 rounding midpoint on the side that turns its row away from (or towards) the other
row, some of them closer to the midpoint than an f32 ulp — the screen is off by 0.5 ... 0.9 x 2^-7, a large part of the bound that the
kernel's margin delta = 2^-6 is twice of — and what is compared with is
  (a) the model's screen (numpy: f64 -> f32 -> bf16 round-to-nearest-even, sums in f64): |approx_gpu - screen| <= 3 d 2^-24 + 2^-22, the
      kernel comment's own f32 accumulation term plus the final division and square roots;
  (b) exact cosines (integer arithmetic) just above the gate: the device's own screen lies below cosine_min - 2^-8 for some — the margin
      is USED — and every pair above the gate holds the oracle's bits;
  (c) exact cosines below the gate that the screen over-estimates: below the gate on the device, and not live;
  (d) the live list of k_cos_live: the pairs whose exact cosine exceeds cosine_min, and the oracle's single scores bit for bit;
  (e) batches of ragged problems against the oracle's register();
  (f) the edges of the screen's case split: 4095 / 4096 / 4160 candidates, one row holding every candidate, rounded-row norms 2^-20 inside
      and outside [2^-40, 2^40], extreme element spread, 176 and 192 blocks.
Measured on an MI355X: the 41 tests of this module take 4.2 s; the largest |approx_gpu - screen| is 2.7e-7 (d = 515) against the allowed
9.2e-5, the planted screens lie up to 0.0055 (cosine_min 0.5), 0.0046 (0.6) and 0.0072 (0.0) below the gate — DESIGN.md section 4 has the
table per d.  Each test prints its figures before it asserts."""
import functools
import math

import numpy as np
import pytest

import _bf16_screen as m
from conftest import registration_for
from roman_amd import synth
from roman_amd.align import batch as rb

pytestmark = pytest.mark.gpu

SHAPES = [(200, 200, 512), (37, 53, 70), (113, 97, 33), (90, 70, 15), (64, 64, 768), (208, 208, 515), (256, 160, 64), (17, 5, 31)]
GATES = {"default": dict(), "0.6-0.8": dict(cosine_min=0.6, cosine_max=0.8), "zero": dict(cosine_min=0.0)}
NEAR = 2.0 ** -40                   # a cosine of up to 768 terms evaluated in long double is exact to well below this


def _tol(d):
    return m.accumulation_term(d) + 2.0 ** -22


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Case:
    pass


def _reg(ctx, d, gate):
    reg = registration_for("semanticgrav", semantics_dim=d, **GATES[gate]); reg.set_context(ctx)
    return reg


def _background(rng, n, d, cmin, dirn):
    """Rows that share the direction `dirn` loosely: cosines on both sides of the gate, few enough above it for the candidate list."""
    X = rng.standard_normal((n, d))
    if cmin > 0.0:
        X += rng.uniform(0.0, 1.1, size=(n, 1)) * dirn
    return X * np.exp2(rng.integers(-3, 4, size=(n, 1)))


def _plant(rng, c, D1, D2, lo, d, cmin, per_side):
    """Adversarial pairs on distinct rows of both maps, the last row of each map among them; under-estimated ones just above the gate
    (half of them within 2^-13 of it), over-estimated ones below it: just below, around cosine_min - 2^-6, and between."""
    n1, n2 = D1.shape[0], D2.shape[0]
    K = min(2 * per_side, n1, n2)
    r1 = np.concatenate([[n1 - 1], rng.permutation(n1 - 1)[:K - 1]]).astype(int)
    r2 = np.concatenate([rng.permutation(n2 - 1)[:K - 1], [n2 - 1]]).astype(int)
    c.plants = []
    for t in range(K):
        sa, sb = 2.0 ** int(rng.integers(-20, 21)), 2.0 ** int(rng.integers(-20, 21))
        if t % 2 == 0:
            a, b = m.adversarial_pair(rng, d, cmin, sa, sb, lo=cmin, hi=cmin + (2.0 ** -13 if t % 4 == 0 else 2.0 ** -10))
            kind = "under"
        else:
            top = [cmin, cmin - m.DELTA, cmin - m.DELTA + 2.0 ** -8][(t // 2) % 3]
            a, b = m.adversarial_pair_up(rng, d, cmin, sa, sb, lo=max(top - 2.0 ** -9, cmin - m.DELTA - m.BOUND), hi=top)
            kind = "over"
        if t % 3 == 2:
            a, b = b, a
        D1[r1[t], lo:lo + d] = a; D2[r2[t], lo:lo + d] = b
        c.plants.append((int(r1[t]), int(r2[t]), kind))


@functools.lru_cache(maxsize=None)
def _case(n1, n2, d, gate, per_side=12):
    reg = registration_for("semanticgrav", semantics_dim=d, **GATES[gate])
    P = reg._abi_params()
    c = Case()
    c.cmin, c.lo, c.d = float(P.cosine_min), P.point_dim + P.ratio_feature_dim, d
    rng = np.random.default_rng(n1 * 1009 + n2 * 13 + d + len(gate))
    pr = synth.make_pair(n1, n2, d, 40 + n1 + n2 + d, tilt_deg=1.0)
    c.D1, c.D2 = reg.pack(pr.map1).copy(), reg.pack(pr.map2).copy()
    dirn = rng.standard_normal(d)
    c.D1[:, c.lo:c.lo + d] = _background(rng, n1, d, c.cmin, dirn); c.D2[:, c.lo:c.lo + d] = _background(rng, n2, d, c.cmin, dirn)
    _plant(rng, c, c.D1, c.D2, c.lo, d, c.cmin, per_side)
    _reference(c)
    return c


def _reference(c):
    """The plain side: the model's screen, long-double cosines of all pairs, exact gate decisions of the planted ones."""
    A, B = c.D1[:, c.lo:c.lo + c.d], c.D2[:, c.lo:c.lo + c.d]
    c.A, c.B = A, B
    c.screen = m.screen_matrix(A, B)
    c.cos = cos = np.asarray(m.cos_matrix(A, B), dtype=np.longdouble)
    c.above = np.asarray(cos > c.cmin + NEAR); c.below = np.asarray(cos < c.cmin - NEAR)
    c.exact = {}
    for i, j, kind in c.plants:
        e = m.exact_cos(A[i], B[j]); g = m.exact_gate(A[i], B[j], c.cmin)
        c.exact[(i, j)] = e
        c.above[i, j], c.below[i, j] = g, (not g) and e < c.cmin
    assert (~(c.above | c.below)).sum() < 0.01 * cos.size
    if -(-A.shape[0] // 16) * -(-B.shape[0] // 16) <= 176:
        assert (c.screen >= c.cmin - m.DELTA).sum() <= 4096, "the case is meant for the screen path"


def _oracle_matrix(orc, c):
    return np.array([[orc.cosine(c.A[i], c.B[j]) for j in range(c.B.shape[0])] for i in range(c.A.shape[0])])


def _three(ctx, monkeypatch, P, D1, D2):
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    dense = ctx.debug_cosine(P, D1, D2)
    monkeypatch.setenv("ROMAN_COS_SEL", "approx")
    approx = ctx.debug_cosine(P, D1, D2)
    monkeypatch.setenv("ROMAN_COS_SEL", "gated")
    gated = ctx.debug_cosine(P, D1, D2)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    return dense, approx, gated


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,d", SHAPES)
def test_a_the_devices_screen_is_the_models(ctx, monkeypatch, n1, n2, d):
    """A truncating (or otherwise different) conversion is off by ~0.005 on the planted rows; so is a one-step f64 -> bf16 on the elements
    that sit closer to a midpoint than an f32 ulp."""
    c = _case(n1, n2, d, "default")
    P = _reg(ctx, d, "default")._abi_params()
    monkeypatch.setenv("ROMAN_COS_SEL", "approx")
    approx = ctx.debug_cosine(P, c.D1, c.D2)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    err = np.abs(approx - c.screen)
    pl = max(err[i, j] for i, j, _ in c.plants)
    under = max(c.exact[(i, j)] - approx[i, j] for i, j, k in c.plants if k == "under")
    over = max([approx[i, j] - c.exact[(i, j)] for i, j, k in c.plants if k == "over"] or [0.0])
    print(f"d = {d} ({n1} x {n2}): max |approx_gpu - screen| = {err.max():.3e} (planted pairs {pl:.3e}) against {_tol(d):.3e}; "
          f"device under-estimate {under / m.BOUND:.3f} x 2^-7, over-estimate {over / m.BOUND:.3f} x 2^-7")
    assert err.max() <= _tol(d)
    assert np.max(np.abs(approx - np.asarray(c.cos, dtype=np.float64))) <= m.BOUND + m.accumulation_term(d)


# ---- (b), (c) ---------------------------------------------------------------------------------------------------------------------------
BC = [(s, "default") for s in SHAPES] + [((37, 53, 70), "0.6-0.8"), ((113, 97, 33), "0.6-0.8"), ((200, 200, 512), "0.6-0.8"), ((90, 70, 15), "0.6-0.8"),
                                         ((37, 53, 70), "zero"), ((90, 70, 15), "zero"), ((64, 64, 768), "zero")]


@pytest.mark.parametrize("shape,gate", BC, ids=[f"{s[0]}x{s[1]}x{s[2]}-{g}" for s, g in BC])
def test_b_c_the_margin_is_used_and_holds_on_both_sides_of_the_gate(ctx, orc, monkeypatch, shape, gate):
    n1, n2, d = shape
    c = _case(n1, n2, d, gate)
    P = _reg(ctx, d, gate)._abi_params()
    dense, approx, gated = _three(ctx, monkeypatch, P, c.D1, c.D2)
    ref = _oracle_matrix(orc, c)
    under = [(i, j) for i, j, k in c.plants if k == "under"]
    over = [(i, j) for i, j, k in c.plants if k == "over"]
    for i, j in under:
        assert c.cmin < c.exact[(i, j)] <= c.cmin + 2.0 ** -10
    for i, j in over:
        assert c.cmin - m.DELTA - m.BOUND <= c.exact[(i, j)] < c.cmin
    # (b) the inputs reach into the margin — a property of the inputs, read off the device's own screen ...
    deepest = min(approx[i, j] for i, j in under)
    print(f"{shape} {gate}: deepest planted screen {c.cmin - deepest:.6f} below the gate ({(c.cmin - deepest) / m.DELTA:.3f} of delta)")
    assert deepest < c.cmin - 2.0 ** -8
    # ... and every pair above the gate — planted or not — holds the oracle's bits
    assert (gated != dense).any()                                      # (the screen path: some pair holds the screen's value)
    assert np.array_equal(_bits(dense), _bits(ref))
    assert np.array_equal(_bits(gated)[c.above], _bits(ref)[c.above])
    for i, j in under:
        assert _bits(gated[i, j]) == _bits(ref[i, j]) and ref[i, j] > c.cmin, (i, j)
    # (c) whatever the screen does below the gate: below the gate
    assert np.all(gated[c.below] < c.cmin)
    for i, j in over:
        assert gated[i, j] < c.cmin, (i, j)
    near = ~(c.above | c.below)                                        # (too close to call in long double: the oracle's side decides)
    assert np.array_equal(gated[near] > c.cmin, ref[near] > c.cmin)


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------
D_CASES = [(s, "default") for s in SHAPES] + [((113, 97, 33), "0.6-0.8"), ((37, 53, 70), "zero")]


@pytest.mark.parametrize("shape,gate", D_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{g}" for s, g in D_CASES])
def test_d_the_live_list_is_the_set_of_pairs_above_the_gate(ctx, orc, monkeypatch, shape, gate):
    n1, n2, d = shape
    c = _case(n1, n2, d, gate)
    P = _reg(ctx, d, gate)._abi_params()
    monkeypatch.setenv("ROMAN_COS_SEL", "1")
    ctx.score(P, c.D1, c.D2)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    idx, sc = ctx.live()
    assert np.all(np.diff(idx) > 0)
    live = np.zeros(n1 * n2, dtype=bool); live[idx] = True
    live = live.reshape(n1, n2)
    assert np.all(live[c.above]) and not np.any(live[c.below])
    for i, j, kind in c.plants:
        assert live[i, j] == (kind == "under"), (i, j, kind)
    s = orc.single_scores(P, c.D1, c.D2)
    assert np.array_equal(idx, np.nonzero(s > 0)[0])
    assert np.array_equal(_bits(sc), _bits(s[idx]))


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------
def _same_as_register(orc, P, res, batch, k):
    D1 = batch.feats[int(batch.off1[k]):int(batch.off1[k]) + int(batch.n1[k])]; D2 = batch.feats[int(batch.off2[k]):int(batch.off2[k]) + int(batch.n2[k])]
    o = orc.register(P, D1, D2)
    st = o["stats"]
    assert np.array_equal(res.assoc[k], o["assoc"]), k
    got = tuple(int(res.stats[f][k]) for f in ("n_live", "nnz_upper", "n_pass", "outer_iters", "inner_iters", "ls_trials"))
    assert got == (st.n_live, st.nnz_upper, st.n_pass, st.outer_iters, st.inner_iters, st.ls_trials), k


@pytest.mark.parametrize("B,nlo,nhi,d,mixed", [(16, 60, 110, 70, True), (40, 30, 90, 33, False)])
def test_e_a_batch_against_the_oracles_register(ctx, orc, monkeypatch, B, nlo, nhi, d, mixed):
    reg = _reg(ctx, d, "default")
    P = reg._abi_params()
    lo, cmin = P.point_dim + P.ratio_feature_dim, float(P.cosine_min)
    rng = np.random.default_rng(B + d)
    pairs = []
    for k in range(B):
        n, n_ = (84, 82) if mixed and k == 3 else (int(rng.integers(nlo, nhi + 1)), int(rng.integers(nlo, nhi + 1)))
        pr = synth.make_pair(n, n_, d, 8100 + 10 * d + k, tilt_deg=1.0)
        pairs.append((pr.map1, pr.map2))
    batch = rb.batch_from_pairs(reg, pairs)
    assert batch.assoc is None
    for k in range(B):
        D1 = batch.feats[int(batch.off1[k]):int(batch.off1[k]) + int(batch.n1[k])]; D2 = batch.feats[int(batch.off2[k]):int(batch.off2[k]) + int(batch.n2[k])]
        if mixed and k == 3:
            # every unplanted pair at cos = 0.493 exactly (disjoint supports but for ten shared coordinates): a candidate, not live —
            # more candidates than the list holds, the problem is left to the dense kernel
            u = np.zeros(d); u[:10] = rng.standard_normal(10); u /= np.linalg.norm(u)
            for D, blk in ((D1, slice(10, 40)), (D2, slice(40, 70))):
                X = np.zeros((D.shape[0], d)); X[:, blk] = rng.standard_normal((D.shape[0], 30))
                X /= np.linalg.norm(X, axis=1, keepdims=True)
                D[:, lo:lo + d] = (math.sqrt(0.493) * u + math.sqrt(1 - 0.493) * X) * rng.uniform(0.5, 2.0, size=(D.shape[0], 1))
        c = Case()
        _plant(rng, c, D1, D2, lo, d, cmin, 8)
        assert len(c.plants) >= 16
        if mixed and k == 3:
            A_, B_ = D1[:, lo:lo + d], D2[:, lo:lo + d]
            assert (m.screen_matrix(A_, B_) >= cmin - m.DELTA).sum() > 4096
        if mixed and k == 5:                                           # rows the screen cannot bound, between the planted ones
            free1 = [r for r in range(D1.shape[0]) if r not in {p[0] for p in c.plants}]
            free2 = [r for r in range(D2.shape[0]) if r not in {p[1] for p in c.plants}]
            D1[free1[0], lo:lo + d] *= 1e150; D1[free1[1], lo:lo + d] *= 2.0 ** 41; D1[free1[2], lo:lo + d] = 0.0
            D2[free2[0], lo:lo + d] *= 1e-150; D2[free2[1], lo:lo + d] *= 2.0 ** -45
    for setting in ("1", "1"):                                         # (the first call of a parameter block sizes its workspace without a history)
        monkeypatch.setenv("ROMAN_COS_SEL", setting)
        with np.errstate(all="ignore"):
            res = rb.run_batch(reg, batch)
    ctx.sync()
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    assert ctx.cosine_screen_stats()[2] == (1 / B if mixed else 0.0)
    assert (res.stats["n_live"] >= 8).all()
    for k in range(B):
        _same_as_register(orc, P, res, batch, k)


# ---- (f) --------------------------------------------------------------------------------------------------------------------------------
def test_f_candidate_counts_at_the_cap(ctx, orc, monkeypatch):
    """Descriptors that are all alike: every pair is a candidate and live.  63 x 65 = 4095 and 64 x 64 = 4096 candidates stay with the screen
    kernel (the list holds 4096), 64 x 65 = 4160 go to the dense kernel; the live list is complete, ascending and the oracle's either way."""
    d = 64
    reg = _reg(ctx, d, "default")
    P = reg._abi_params(); lo = P.point_dim + P.ratio_feature_dim
    for (n1, n2), share in (((63, 65), 0.0), ((64, 64), 0.0), ((64, 65), 1.0)):
        prs = [synth.make_pair(n1, n2, d, 9300 + n1 * n2 + k, tilt_deg=1.0) for k in range(2)]
        batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in prs])
        batch.feats[:, lo:lo + d] = 1.0 + 0.01 * np.random.default_rng(n1 * n2).standard_normal((batch.feats.shape[0], d))
        monkeypatch.setenv("ROMAN_COS_SEL", "1")
        res = rb.run_batch(reg, batch); ctx.sync()
        assert ctx.cosine_screen_stats()[2] == share, (n1, n2)
        assert (res.stats["n_live"] == n1 * n2).all()
        D1 = batch.feats[int(batch.off1[0]):int(batch.off1[0]) + n1]; D2 = batch.feats[int(batch.off2[0]):int(batch.off2[0]) + n2]
        ctx.score(P, D1, D2)
        monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
        idx, sc = ctx.live()
        s = orc.single_scores(P, D1, D2)
        assert np.array_equal(idx, np.arange(n1 * n2)) and (s > 0).all()
        assert np.array_equal(_bits(sc), _bits(s))


def test_f_every_candidate_in_one_row(ctx, orc, monkeypatch):
    """One object of map 1 is like all 256 of map 2, the others share no coordinate with them: one bucket of 256 in the sort by row."""
    d, n1, n2, row = 64, 100, 256, 77
    reg = _reg(ctx, d, "default")
    P = reg._abi_params(); lo = P.point_dim + P.ratio_feature_dim
    rng = np.random.default_rng(5)
    pr = synth.make_pair(n1, n2, d, 9400, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1).copy(), reg.pack(pr.map2).copy()
    u = rng.standard_normal(32)
    D1[:, lo:lo + d] = 0.0; D2[:, lo:lo + d] = 0.0
    D1[:, lo + 32:lo + d] = rng.standard_normal((n1, 32))
    D1[row, lo:lo + d] = 0.0; D1[row, lo:lo + 32] = u
    D2[:, lo:lo + 32] = u + 0.05 * rng.standard_normal((n2, 32))
    monkeypatch.setenv("ROMAN_COS_SEL", "1")
    ctx.score(P, D1, D2)
    idx, sc = ctx.live()
    monkeypatch.setenv("ROMAN_COS_SEL", "gated")
    gated = ctx.debug_cosine(P, D1, D2)
    monkeypatch.delenv("ROMAN_COS_SEL", raising=False)
    s = orc.single_scores(P, D1, D2)
    assert np.array_equal(idx, row * n2 + np.arange(n2))
    assert np.array_equal(_bits(sc), _bits(s[idx])) and (s > 0).sum() == n2
    assert np.array_equal(_bits(gated[row]), _bits(np.array([orc.cosine(D1[row, lo:lo + d], D2[j, lo:lo + d]) for j in range(n2)])))
    assert np.all(np.delete(gated, row, axis=0) == 0.0)


def test_f_norms_just_inside_and_just_outside_the_trusted_range(ctx, orc, monkeypatch):
    """The case split reads the SCREEN's norm — the f32-accumulated norm of the rounded row — against [2^-40, 2^40].  The planted rows' rounded
    norms lie 2^-20 (relative) inside and 1.25 x 2^-20 outside either end: with 11 elements the f32 accumulation moves the sum of squares by
    at most 11 x 2^-23 < 2^-19 of itself even if every operation truncates, the distance of the sum of squares from 2^+-80.  Inside: the
    screen is trusted — the model's tolerance and the gate hold; outside: the dense kernel's bits for the whole row / column."""
    d0, n1, n2 = 7, 40, 24
    d = d0 + 4
    reg = _reg(ctx, d, "default")
    P = reg._abi_params(); lo, cmin = P.point_dim + P.ratio_feature_dim, float(P.cosine_min)
    rng = np.random.default_rng(6)
    pr = synth.make_pair(n1, n2, d, 9500, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1).copy(), reg.pack(pr.map2).copy()
    dirn = rng.standard_normal(d)
    D1[:, lo:lo + d] = _background(rng, n1, d, cmin, dirn); D2[:, lo:lo + d] = _background(rng, n2, d, cmin, dirn)
    inside_hi, outside_hi = 2.0 ** 80 * (1 - 2.0 ** -20) ** 2, 2.0 ** 80 * (1 + 2.0 ** -20) ** 2 * (1 + 2.0 ** -21)
    outside_lo, inside_lo = 2.0 ** -80 * (1 - 2.0 ** -20) ** 2, 2.0 ** -80 * (1 + 2.0 ** -20) ** 2 * (1 + 2.0 ** -21)
    rows = []                                                          # (map, row of the edge descriptor, row of its partner, inside?)
    for t, (top, inside) in enumerate([(inside_hi, True), (outside_hi, False), (outside_lo, False), (inside_lo, True)] * 2):
        a, b = m.adversarial_pair(rng, d0, cmin, norm2_a=top, lo=cmin, hi=cmin + 2.0 ** -10)
        n = float(m.screen_norms(a))
        assert (2.0 ** -40 * (1 + 2.0 ** -20) <= n <= 2.0 ** 40 * (1 - 2.0 ** -20)) == inside
        assert inside or n >= 2.0 ** 40 * (1 + 2.0 ** -20) or n <= 2.0 ** -40 * (1 - 2.0 ** -20)
        assert m.exact_gate(a, b, cmin)
        if t < 4:
            D1[3 + 9 * t if t < 3 else n1 - 1, lo:lo + d] = a; D2[2 + 5 * t, lo:lo + d] = b
            rows.append((1, 3 + 9 * t if t < 3 else n1 - 1, 2 + 5 * t, inside))
        else:
            t -= 4
            D2[4 + 5 * t if t < 3 else n2 - 1, lo:lo + d] = a; D1[5 + 9 * t, lo:lo + d] = b
            rows.append((2, 4 + 5 * t if t < 3 else n2 - 1, 5 + 9 * t, inside))
    dense, approx, gated = _three(ctx, monkeypatch, P, D1, D2)
    A, B = D1[:, lo:lo + d], D2[:, lo:lo + d]
    scr = m.screen_matrix(A, B)
    trusted = np.ones((n1, n2), dtype=bool)
    for which, r, p, inside in rows:
        sl = (r, slice(None)) if which == 1 else (slice(None), r)
        if not inside:
            trusted[sl] = False
            assert np.array_equal(_bits(approx[sl]), _bits(dense[sl])), (which, r)
            assert np.array_equal(_bits(gated[sl]), _bits(dense[sl])), (which, r)
    assert np.max(np.abs(approx - scr)[trusted]) <= _tol(d)
    for which, r, p, inside in rows:
        i, j = (r, p) if which == 1 else (p, r)
        assert _bits(gated[i, j]) == _bits(orc.cosine(A[i], B[j])) and gated[i, j] > cmin, (which, r)
        if inside:
            assert approx[i, j] < cmin - 2.0 ** -9                     # (d = 11: the family reaches less far than at d >= 15)
    assert (gated != dense).any()


def test_f_safe_norms_with_an_extreme_spread_of_the_elements(ctx, orc, monkeypatch):
    """One element at 2^39 and the others from 2^-60 down to subnormal f32 values; a row of norm ~2^-39 whose small elements (2^-140 ...) are
    zeros in bf16: what is lost stays below 2^-86 of the product of the norms — (a) and (b) hold."""
    d, n1, n2 = 64, 20, 20
    reg = _reg(ctx, d, "default")
    P = reg._abi_params(); lo, cmin = P.point_dim + P.ratio_feature_dim, float(P.cosine_min)
    rng = np.random.default_rng(8)
    pr = synth.make_pair(n1, n2, d, 9600, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1).copy(), reg.pack(pr.map2).copy()
    dirn = rng.standard_normal(d)
    D1[:, lo:lo + d] = _background(rng, n1, d, cmin, dirn); D2[:, lo:lo + d] = _background(rng, n2, d, cmin, dirn)
    spread = rng.choice([-1.0, 1.0], size=d) * np.exp2(-rng.uniform(60, 149, size=d)); spread[11] = 2.0 ** 39
    target = cmin + 2.0 ** -11
    for j in (3, n2 - 1):                                              # partners: cos = b_11 / |b| (to 2^-99)
        b = 0.1 * rng.standard_normal(d); b[11] = 0.0
        b[11] = target * np.linalg.norm(b) / math.sqrt(1 - target * target)
        D2[j, lo:lo + d] = b
    D1[7, lo:lo + d] = spread
    a, b = m.adversarial_pair(rng, 32, cmin, scale_a=2.0 ** -39, scale_b=1.0)
    tail = rng.choice([-1.0, 1.0], size=32) * np.exp2(-rng.uniform(140, 149, size=32))
    D1[n1 - 1, lo:lo + d] = np.concatenate([a, tail]); D2[9, lo:lo + d] = np.concatenate([b, np.zeros(32)])
    dense, approx, gated = _three(ctx, monkeypatch, P, D1, D2)
    A, B = D1[:, lo:lo + d], D2[:, lo:lo + d]
    assert np.max(np.abs(approx - m.screen_matrix(A, B))) <= _tol(d)
    for i, j in ((7, 3), (7, n2 - 1), (n1 - 1, 9)):
        assert m.exact_gate(A[i], B[j], cmin)
        assert _bits(gated[i, j]) == _bits(orc.cosine(A[i], B[j])) and gated[i, j] > cmin, (i, j)
    assert approx[n1 - 1, 9] < cmin - 2.0 ** -8
    cos = np.asarray(m.cos_matrix(A, B))
    ref = np.array([[orc.cosine(A[i], B[j]) for j in range(n2)] for i in range(n1)])
    assert np.array_equal(_bits(gated)[cos > cmin + NEAR], _bits(ref)[cos > cmin + NEAR])
    assert np.all(gated[cos < cmin - NEAR] < cmin)


@pytest.mark.parametrize("n2,screened", [(176, True), (177, False)])
def test_f_maps_at_the_block_budget(ctx, orc, monkeypatch, n2, screened):
    """256 x 176 objects are 16 x 11 = 176 blocks of 16 x 16, the most the screen kernel takes; 256 x 177 are 192: the dense kernel."""
    n1, d = 256, 32
    c = _case(n1, n2, d, "default", 8)
    P = _reg(ctx, d, "default")._abi_params()
    dense, approx, gated = _three(ctx, monkeypatch, P, c.D1, c.D2)
    ref = _oracle_matrix(orc, c)
    assert np.array_equal(_bits(dense), _bits(ref))
    if screened:
        assert np.max(np.abs(approx - c.screen)) <= _tol(d)
        assert min(approx[i, j] for i, j, k in c.plants if k == "under") < c.cmin - 2.0 ** -8
        assert (gated != dense).any()
        assert np.array_equal(_bits(gated)[c.above], _bits(ref)[c.above]) and np.all(gated[c.below] < c.cmin)
    else:
        assert np.array_equal(_bits(approx), _bits(dense)) and np.array_equal(_bits(gated), _bits(dense))
