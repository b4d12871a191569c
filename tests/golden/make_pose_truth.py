#!/usr/bin/env python3
"""Generate tests/golden/pose_truth.npz: the rigid fit (Arun / Kabsch, unit weights, no scale) of point pairs at the EDGES of the
device's pose code, evaluated on the exact float64 inputs with mpmath at 80 digits.  Re-run with:
    python tests/golden/make_pose_truth.py
Needs numpy and mpmath only; the tests read the committed .npz and need neither this script nor mpmath (tests/test_pose_truth_cpu.py
re-evaluates three cases through `truth()` where mpmath imports).

What is stored, per case (arrays over the cases, in batch order; a case's points are p1[off[i]:off[i+1]].reshape(k, dim)):
    tag, family, dim, k, kind (DETERMINED / UNDETERMINED / INSUFFICIENT: k < dim)
    m1, m2      centroids                                        (the exact value rounded to float64, as everything below)
    H           centred cross-covariance  sum (p1 - m1)(p2 - m2)'
    sv          singular values of H (mpmath.svd_r), descending
    sgn         sign of det H  (0 where H is singular to 60 digits)
    R, t        R = U Vh with the last row of Vh negated when det(U Vh) < 0 (the reference's rule), t = m1 - R m2
    res         the optimal residual  || R p2 + t - p1 ||  (Frobenius norm over all points)
    kappa       conditioning of R: 3-D  s1 / (s2 + sgn s3);  2-D  max(1, s1 / (s1 + sgn s2))      (determined cases)
    c, r        largest absolute coordinate of p1 and p2;  RMS radius of the centred p2

An UNDETERMINED case has rank H <= 1 in 3-D (or is so within what float64 sums of products can hold): the rotation about the line
is free, R and t hold ONE optimal member, and only res and the centroids are meant to be compared.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pose_truth.npz")
DPS = 80
DETERMINED, UNDETERMINED, INSUFFICIENT = 0, 1, 2
SEED = 20261019


# ---------------------------------------------------------------------------------------------- the truth (mpmath)
def _f(x):
    """mpf -> float64, rounded to nearest (float(mpf) truncates)."""
    from mpmath import libmp
    return libmp.to_float(x._mpf_, rnd='n')


def truth(p1, p2, dim):
    """The exact-input fit of p1 ~ R p2 + t, every output rounded once to float64."""
    import mpmath as mp
    with mp.workdps(DPS):
        k = len(p1)
        A = [[mp.mpf(float(v)) for v in row] for row in np.asarray(p1, dtype=np.float64).reshape(k, dim)]
        Q = [[mp.mpf(float(v)) for v in row] for row in np.asarray(p2, dtype=np.float64).reshape(k, dim)]
        m1 = [mp.fsum(a[c] for a in A) / k for c in range(dim)]
        m2 = [mp.fsum(q[c] for q in Q) / k for c in range(dim)]
        H = mp.matrix(dim, dim)
        for r in range(dim):
            for c in range(dim):
                H[r, c] = mp.fsum((a[r] - m1[r]) * (q[c] - m2[c]) for a, q in zip(A, Q))
        hmax = max(abs(H[r, c]) for r in range(dim) for c in range(dim))
        if hmax == 0:                                              # H == 0: every rotation is optimal; the identity is stored
            U, S, Vh = mp.eye(dim), mp.matrix(dim, 1), mp.eye(dim)
        else:
            U, S, Vh = mp.svd_r(H, compute_uv=True)
        assert all(S[i] >= S[i + 1] for i in range(dim - 1))
        if mp.det(U * Vh) < 0:
            for c in range(dim):
                Vh[dim - 1, c] = -Vh[dim - 1, c]
        R = U * Vh
        t = [m1[r] - mp.fsum(R[r, c] * m2[c] for c in range(dim)) for r in range(dim)]
        res2 = mp.mpf(0)
        for a, q in zip(A, Q):
            for r in range(dim):
                res2 += (mp.fsum(R[r, c] * q[c] for c in range(dim)) + t[r] - a[r]) ** 2
        dH = mp.det(H) if hmax else mp.mpf(0)
        sgn = 0 if abs(dH) <= mp.mpf(10) ** -60 * hmax ** dim else (1 if dH > 0 else -1)
        r2 = mp.fsum((q[c] - m2[c]) ** 2 for q in Q for c in range(dim)) / k
        pad = lambda v: np.array([_f(x) for x in v] + [0.0] * (3 - dim))
        M = lambda X: np.array([[_f(X[r, c]) if (r < dim and c < dim) else 0.0 for c in range(3)] for r in range(3)])
        return dict(m1=pad(m1), m2=pad(m2), H=M(H), sv=pad([S[i] for i in range(dim)]), sgn=int(sgn), R=M(R), t=pad(t),
                    res=_f(mp.sqrt(res2)), r=_f(mp.sqrt(r2)))


def kappa_of(sv, sgn, dim):
    if dim == 3:
        return sv[0] / (sv[1] + sgn * sv[2])
    return max(1.0, sv[0] / (sv[0] + sgn * sv[1]))


# ---------------------------------------------------------------------------------------------- the families
def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def rot2(th):
    return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def build_cases():
    """[(family, tag, dim, kind, p1, p2)] in batch order (the 2-D and the 3-D cases are batched separately, each in this order)."""
    rng = np.random.default_rng(SEED)
    cases = []

    def add(family, tag, dim, kind, p1, p2):
        cases.append((family, tag, dim, kind, np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, dim),
                      np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, dim)))

    def general():                                                 # a rotation in general position and a translation
        return rot(rng.standard_normal(3), rng.uniform(0.3, np.pi - 0.3) * rng.choice([-1.0, 1.0])), rng.uniform(-5, 5, 3)

    def rigid3(k, box=15.0, sigma=0.05, scale=1.0, shift2=0.0, shift1=0.0):
        R, t = general()
        p2 = rng.uniform(-box, box, (k, 3)) * scale + shift2
        return (R @ p2.T).T + t * scale + sigma * scale * rng.standard_normal((k, 3)) + shift1, p2

    def short(tag, dim, k):                                        # k < dim: INSUFFICIENT, wherever it sits in the batch
        add("batch", tag, dim, INSUFFICIENT, rng.uniform(-1, 1, (k, dim)), rng.uniform(-1, 1, (k, dim)))

    far_dir = np.array([1.0, -0.7, 0.01])

    # ---- 3-D ------------------------------------------------------------------------------------------------------------
    short("batch3d_first_k0", 3, 0)
    for k in (3, 4, 63, 64, 65, 127, 128, 129, 192, 193, 1000):    # the KEEP = 2 register window of wave_pose ends at 128
        add("window", f"window_k{k}", 3, DETERMINED, *rigid3(k))
        if k == 65:
            short("batch3d_mid_k1", 3, 1)
    short("batch3d_mid_k2", 3, 2)
    for off in (1e3, 1e5, 1e7):                                    # world-frame maps: both clouds far from the origin
        for k in (40, 129):
            add("far", f"far_k{k}_off{off:.0e}", 3, DETERMINED, *rigid3(k, shift2=off * far_dir))
    add("far", "far_p1only_k40_off1e+07", 3, DETERMINED, *rigid3(40, shift1=1e7 * far_dir))   # the rotation acts near the origin, t is large
    short("batch3d_mid_k0", 3, 0)
    for s in (1e-6, 1e-3, 1e3, 1e6):
        add("scale", f"scale_{s:.0e}", 3, DETERMINED, *rigid3(50, scale=s))

    def slab(k, extents, noise):                                   # a box of the given extents, randomly oriented, then moved rigidly
        Q, _ = general()
        p2 = (Q @ (rng.uniform(-1, 1, (k, 3)) * np.asarray(extents)).T).T + rng.uniform(-2, 2, 3)
        R, t = general()
        return (R @ p2.T).T + t + noise * rng.standard_normal((k, 3)), p2

    for f in (1e-2, 1e-4, 1e-6, 1e-8):
        add("flat", f"flat_f{f:.0e}", 3, DETERMINED, *slab(60, (1.0, 0.3, f), 1e-3 * f))
    # exactly planar: p2 = o + a e1 + b e2 with dyadic a, b and dyadic, tilted e1, e2 — no rounding, H has an exact null vector that
    # is no coordinate axis; the rotation is about an axis that is not the plane's normal
    ab = rng.integers(-8192, 8193, (30, 2)) / 1024.0
    p2 = np.array([1.0, -2.0, 0.5]) + np.outer(ab[:, 0], [1.0, 0.0, 0.5]) + np.outer(ab[:, 1], [0.0, 1.0, 0.25])
    R, t = general()
    add("flat", "planar_tilted", 3, DETERMINED, (R @ p2.T).T + t, p2)
    for h in (1e-2, 1e-4):                                         # determined, ill-conditioned: kappa ~ 1 / h^2
        add("needle", f"needle_h{h:.0e}", 3, DETERMINED, *slab(60, (1.0, h, h / 2), 1e-3 * h))

    cube = np.array([[x, y, z] for x in (-2.0, 2.0) for y in (-2.0, 2.0) for z in (-2.0, 2.0)]) + np.array([1.0, -2.0, 0.5])
    R, t = general()
    add("equal", "cube_rotated", 3, DETERMINED, (R @ cube.T).T + t, cube)                 # s1 = s2 = s3 up to the rounding of p1
    add("equal", "cube_identity", 3, DETERMINED, cube.copy(), cube)                       # H = 32 I exactly
    axes = np.concatenate([2.0 * np.eye(3), -2.0 * np.eye(3)])
    add("equal", "axes6_identity", 3, DETERMINED, axes.copy(), axes)                      # H = 8 I: no sweep moves
    add("equal", "axes6_pi", 3, DETERMINED, axes * np.array([-1.0, -1.0, 1.0]), axes)     # H = diag(-8, -8, 8): a turn by pi about z
    # an axis reflection, H = diag(-18, 8, 2): unequal extents, because with equal ones the direction that the reflection fix
    # gives up is not unique.  The optimum turns by pi about y: it gives up the SMALLEST direction, not the mirrored one.
    ax3 = np.concatenate([np.diag([3.0, 2.0, 1.0]), -np.diag([3.0, 2.0, 1.0])])
    add("equal", "axes6_reflected", 3, DETERMINED, ax3 * np.array([-1.0, 1.0, 1.0]), ax3)

    for k in (4, 50, 129):                                         # a mirrored cloud, then rotated: det H < 0 in general position
        p2 = rng.uniform(-10, 10, (k, 3))
        R, t = general()
        add("reflect", f"reflect_k{k}", 3, DETERMINED, (R @ (p2 * np.array([1.0, 1.0, -1.0])).T).T + t + 0.01 * rng.standard_normal((k, 3)), p2)

    short("batch3d_mid2_k1", 3, 1)
    for k in (3, 65):                                              # one line in general position: the turn about it is free
        dirn = rng.standard_normal(3); dirn /= np.linalg.norm(dirn)
        p2 = np.outer(np.sort(rng.uniform(-12, 12, k)), dirn) + np.array([1.0, -2.0, 0.5])
        R, t = general()
        add("undetermined", f"collinear_k{k}", 3, UNDETERMINED, (R @ p2.T).T + t, p2)
    add("undetermined", "needle_h1e-09", 3, UNDETERMINED, *slab(60, (1.0, 1e-9, 5e-10), 1e-12))   # s2 / s1 ~ 1e-18: below what a float64 H holds
    a, b = rng.uniform(-15, 15, 3), rng.uniform(-15, 15, 3)
    add("undetermined", "identical", 3, UNDETERMINED, np.tile(a, (5, 1)), np.tile(b, (5, 1)))
    add("undetermined", "p2_identical", 3, UNDETERMINED, rng.uniform(-15, 15, (6, 3)), np.tile(b, (6, 1)))
    # the same past the 128-pair register window, where a third sweep over the points has to fetch them again.  (A stream of their
    # own: the cases above and below stay what they were before these were added.)
    rng_main, rng = rng, np.random.default_rng(SEED + 1)
    for k in (129, 200):
        add("undetermined", f"needle_h1e-09_k{k}", 3, UNDETERMINED, *slab(k, (1.0, 1e-9, 5e-10), 1e-12))
    dirn = rng.standard_normal(3); dirn /= np.linalg.norm(dirn)
    p2 = np.outer(np.sort(rng.uniform(-12, 12, 129)), dirn) + np.array([1.0, -2.0, 0.5])
    R, t = general()
    add("undetermined", "collinear_k129", 3, UNDETERMINED, (R @ p2.T).T + t, p2)
    rng = rng_main
    short("batch3d_last_k2", 3, 2)
    short("batch3d_last_k0", 3, 0)

    # ---- 2-D ------------------------------------------------------------------------------------------------------------
    def rigid2(k, sigma=0.05, shift2=0.0):
        p2 = rng.uniform(-15, 15, (k, 2)) + shift2
        return (rot2(rng.uniform(-np.pi, np.pi)) @ p2.T).T + rng.uniform(-5, 5, 2) + sigma * rng.standard_normal((k, 2)), p2

    short("batch2d_first_k0", 2, 0)
    for k in (2, 3, 64, 65, 129):
        add("2d", f"rigid2d_k{k}", 2, DETERMINED, *rigid2(k))
        if k == 64:
            short("batch2d_mid_k1", 2, 1)
    p2 = rng.uniform(-10, 10, (20, 2))
    add("2d", "reflect2d_k20", 2, DETERMINED, (rot2(rng.uniform(-np.pi, np.pi)) @ (p2 * np.array([1.0, -1.0])).T).T + rng.uniform(-5, 5, 2)
        + 0.01 * rng.standard_normal((20, 2)), p2)
    short("batch2d_mid_k0", 2, 0)
    dirn = rng.standard_normal(2); dirn /= np.linalg.norm(dirn)    # rank-1 H: in 2-D the proper rotation is still determined
    p2 = np.outer(np.sort(rng.uniform(-12, 12, 10)), dirn) + np.array([1.0, -2.0])
    add("2d", "collinear2d_k10", 2, DETERMINED, (rot2(rng.uniform(-np.pi, np.pi)) @ p2.T).T + rng.uniform(-5, 5, 2), p2)
    add("2d", "far2d_k40_off1e+05", 2, DETERMINED, *rigid2(40, shift2=1e5 * far_dir[:2]))
    short("batch2d_last_k1", 2, 1)
    short("batch2d_last_k0", 2, 0)
    return cases


#: what tests/test_pose_truth_cpu.py expects to find: family -> number of cases
FAMILY_COUNTS = {"window": 11, "far": 7, "scale": 4, "flat": 5, "needle": 2, "equal": 5, "reflect": 3, "2d": 8, "undetermined": 8,
                 "batch": 12}


def main():
    cases = build_cases()
    n = len(cases)
    out = dict(tag=np.array([c[1] for c in cases]), family=np.array([c[0] for c in cases]),
               dim=np.array([c[2] for c in cases], dtype=np.int32), kind=np.array([c[3] for c in cases], dtype=np.int32),
               k=np.array([len(c[4]) for c in cases], dtype=np.int64))
    out["off"] = np.concatenate([[0], np.cumsum(out["k"] * out["dim"])]).astype(np.int64)
    out["p1"] = np.concatenate([c[4].ravel() for c in cases]); out["p2"] = np.concatenate([c[5].ravel() for c in cases])
    for name, shape in (("m1", (3,)), ("m2", (3,)), ("H", (3, 3)), ("sv", (3,)), ("R", (3, 3)), ("t", (3,))):
        out[name] = np.full((n,) + shape, np.nan)
    for name in ("res", "kappa", "c", "r"):
        out[name] = np.full(n, np.nan)
    out["sgn"] = np.zeros(n, dtype=np.int32)
    for i, (family, tag, dim, kind, p1, p2) in enumerate(cases):
        if kind == INSUFFICIENT:
            continue
        tr = truth(p1, p2, dim)
        for name in ("m1", "m2", "H", "sv", "R", "t", "res", "r", "sgn"):
            out[name][i] = tr[name]
        out["c"][i] = max(np.abs(p1).max(), np.abs(p2).max())
        if kind == DETERMINED:
            out["kappa"][i] = kappa_of(tr["sv"], tr["sgn"], dim)
        print(f"  {tag:26s} dim={dim} k={len(p1):4d} sv={tr['sv'][:dim]} sgn={tr['sgn']:+d} kappa={out['kappa'][i]:.3g} "
              f"c={out['c'][i]:.3g} r={tr['r']:.3g} res={tr['res']:.3g}")
    fam, cnt = np.unique(out["family"], return_counts=True)
    assert dict(zip(fam.tolist(), cnt.tolist())) == FAMILY_COUNTS, dict(zip(fam.tolist(), cnt.tolist()))
    np.savez_compressed(OUT, **out)
    print(f"pose_truth.npz: {n} cases, {out['k'].sum()} point pairs, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
