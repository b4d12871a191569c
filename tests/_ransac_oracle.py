"""NumPy restatement of the deterministic RANSAC registration of DESIGN.md §4.7 (roman_ransac_batch in include/roman_hip.h),
steps 1-7: Python integers for the draws, numpy.linalg.svd Kabsch with the determinant fix for the three-point fits, the
repository's pose oracle (oracle.t_align) for the final Arun fit.

The device's Kabsch and NumPy's differ by rounding, so a comparison is exact only away from the thresholds: every hypothesis
carries a BORDERLINE flag, set when a squared distance lies within 1e-9 of max_dist^2 or an edge test within 1e-9 of equality.
Tests assert that their seeds and shapes have none."""
import math
from types import SimpleNamespace

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
BORDER = 1e-9


def mix64(z):
    """The published splitmix64 finaliser."""
    z &= MASK64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def draw(seed, c):
    """Output c + 1 of splitmix64 seeded with `seed`."""
    return mix64((seed + (c + 1) * GOLDEN) & MASK64)


def mulhi64(a, b):
    return (a * b) >> 64


def sample(seed, h, n, m):
    """The three correspondences (i_k, j_k) of hypothesis h."""
    out = []
    for k in range(3):
        a = mulhi64(draw(seed, 3 * h + k), n * m)
        out.append((a // m, a % m))
    return out


def kabsch(src, dst):
    """Rigid transform (no scale) with R src + t ~ dst."""
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    H = (dst - md).T @ (src - ms)
    U, _, Vh = np.linalg.svd(H)
    R = U @ Vh
    if np.linalg.det(R) < 0:
        Vh = Vh.copy(); Vh[-1, :] *= -1.0
        R = U @ Vh
    return R, md - R @ ms


def stop_estimate(best_count, nm, max_iteration, confidence):
    """K of step 6."""
    if best_count <= 0:
        return max_iteration
    f = best_count / nm
    if f >= 1.0:
        return 0
    den = math.log(1.0 - f * f * f)
    if den == 0.0:
        return max_iteration
    return min(max_iteration, math.ceil(math.log(1.0 - confidence) / den))


def hypothesis(P, Q, seed, h, edge_len, max_dist):
    """-> (pruned, count, sse, borderline, D2 or None) of hypothesis h."""
    n, m = len(P), len(Q)
    s = sample(seed, h, n, m)
    ii = [a for a, _ in s]; jj = [b for _, b in s]
    if len(set(ii)) < 3 or len(set(jj)) < 3:
        return True, -1, 0.0, False, None
    border, pruned = False, False
    for k in range(3):
        l = (k + 1) % 3
        ds = float(np.linalg.norm(P[ii[k]] - P[ii[l]])); dt = float(np.linalg.norm(Q[jj[k]] - Q[jj[l]]))
        if abs(ds - dt * edge_len) < BORDER or abs(dt - ds * edge_len) < BORDER:
            border = True
        if ds < dt * edge_len or dt < ds * edge_len:
            pruned = True
    if pruned:
        return True, -1, 0.0, border, None
    R, t = kabsch(P[ii], Q[jj])
    TP = P @ R.T + t
    D2 = ((TP[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2)           # (n, m): row-major = the correspondence order
    md2 = max_dist * max_dist
    if np.any(np.abs(D2 - md2) < BORDER):
        border = True
    inl = D2 < md2
    return False, int(inl.sum()), float(D2[inl].sum()), border, D2


def run(P, Q, max_iteration=2048, round=256, edge_len=0.95, max_dist=0.5, confidence=0.999, seed=0):
    """Steps 1-6 -> namespace(counts (n_hyp,) int32 with -1 = pruned, sse, n_hyp, n_scored, n_border, best_count,
    best_set (the hypotheses with the best count whose sse is within 1e-9 relative of the smallest), triples)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3); Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    n, m = len(P), len(Q)
    counts, sses = [], []
    n_border = 0
    best = -1
    done = 0
    while True:
        end = min(done + round, max_iteration)
        for h in range(done, end):
            pruned, c, s, bd, _ = hypothesis(P, Q, seed, h, edge_len, max_dist)
            counts.append(-1 if pruned else c); sses.append(s)
            n_border += bool(bd)
            if not pruned:
                best = max(best, c)
        done = end
        if done >= max_iteration or done >= stop_estimate(best, n * m, max_iteration, confidence):
            break
    counts = np.array(counts, dtype=np.int32); sses = np.array(sses)
    best_set = []
    if best >= 0:
        cand = np.nonzero(counts == best)[0]
        smin = sses[cand].min()
        best_set = [int(h) for h in cand if sses[h] <= smin + 1e-9 * max(smin, 1e-300)]
    return SimpleNamespace(counts=counts, sse=sses, n_hyp=done, n_scored=int((counts >= 0).sum()), n_border=n_border,
                           best_count=max(best, 0), best_set=best_set, P=P, Q=Q,
                           params=dict(edge_len=edge_len, max_dist=max_dist, seed=seed))


def same_triple(res, hs):
    """Do the hypotheses `hs` all sample the same three correspondences (in any order)?"""
    n, m = len(res.P), len(res.Q)
    keys = {tuple(sorted(sample(res.params["seed"], h, n, m))) for h in hs}
    return len(keys) <= 1


def inlier_rows(res, h):
    """(k, 2) int32 inlier rows of hypothesis h, row-major order, and its sse."""
    pruned, c, s, _, D2 = hypothesis(res.P, res.Q, res.params["seed"], h, res.params["edge_len"], res.params["max_dist"])
    assert not pruned
    rows = np.argwhere(D2 < res.params["max_dist"] ** 2).astype(np.int32)
    assert len(rows) == c
    return rows, s


def pose_on(orc, P, Q, rows):
    """Arun on the rows, map 2 -> map 1 (the inherited T_align)."""
    return orc.t_align(np.asarray(P)[rows[:, 0]], np.asarray(Q)[rows[:, 1]], 3)


def result(orc, P, Q, **kw):
    """Steps 1-7 with the oracle's own winner (lowest index of the best set) -> (rows, T or None, run namespace)."""
    res = run(P, Q, **kw)
    if not res.best_set:
        return np.zeros((0, 2), np.int32), None, res
    rows, _ = inlier_rows(res, res.best_set[0])
    return rows, (pose_on(orc, res.P, res.Q, rows) if len(rows) >= 3 else None), res


def planted(n, m, seed, n_in=None, noise=0.01, box=10.0):
    """P: n random points in a `box` m cube.  Q: the first n_in of them carried by a rigid motion (R P + t) with Gaussian noise,
    the other m - n_in fresh random points; Q is then shuffled.  -> (P, Q, R, t, truth rows (i, j) sorted by i)."""
    rng = np.random.default_rng(seed)
    n_in = min(n, m) if n_in is None else n_in
    P = rng.uniform(0.0, box, (n, 3))
    ang = rng.uniform(-np.pi, np.pi); ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    t = rng.uniform(-3.0, 3.0, 3)
    Q = np.vstack([P[:n_in] @ R.T + t + noise * rng.normal(size=(n_in, 3)), rng.uniform(0.0, box, (m - n_in, 3)) @ R.T + t])
    perm = rng.permutation(m)
    Qs = np.empty_like(Q); Qs[perm] = Q                                # Q[k] lands at index perm[k]
    truth = np.array([(i, perm[i]) for i in range(n_in)], dtype=np.int32)
    return P, Qs, R, t, truth


class _Seg:
    """The one attribute RansacReg reads from an object."""

    def __init__(self, c, id=0):
        self.center = np.asarray(c, dtype=np.float64).reshape(3, 1)
        self.id = id


def segments(points, id0=0):
    return [_Seg(p, id0 + k) for k, p in enumerate(np.asarray(points).reshape(-1, 3))]


def compute_double(orc):
    """A `compute` for submap_align built from this oracle: (registration, AlignmentBatch) -> the fields of runtime.RansacResult
    the pair loop reads."""
    from roman_amd import _abi

    def compute(registration, batch):
        assoc, Ts, status = [], [], []
        for b in range(len(batch)):
            P = batch.feats[batch.off1[b]:batch.off1[b] + batch.n1[b]]; Q = batch.feats[batch.off2[b]:batch.off2[b] + batch.n2[b]]
            if len(P) == 0 or len(Q) == 0:
                assoc.append(np.zeros((0, 2), np.int32)); Ts.append(np.full((4, 4), np.nan)); status.append(_abi.ROMAN_ST_EMPTY_MAP)
                continue
            rows, T, res = result(orc, P, Q, max_iteration=registration.max_iteration, round=registration.round, edge_len=registration.edge_len,
                                  max_dist=registration.max_dist, confidence=registration.confidence, seed=registration.seed)
            assert res.n_border == 0 and len(res.best_set) <= 1, "the double is exact only away from the thresholds"
            assoc.append(rows); Ts.append(np.full((4, 4), np.nan) if T is None else T)
            status.append(_abi.ROMAN_ST_INSUFFICIENT if T is None else _abi.ROMAN_ST_OK)
        return SimpleNamespace(assoc=assoc, T=np.array(Ts).reshape(-1, 4, 4), status=np.array(status, dtype=np.int32))
    return compute
