"""Pass 1 of the pair loop over an S0 x S1 grid, restated in NumPy — TEST INFRASTRUCTURE: the expectation for roman_grid_gate_dev /
roman_grid_gate (include/roman_hip.h) and the stand-in's gate in tests/test_grid_gate_cpu.py.

A side is a dict: pos (S, 3), pos_gt (S, 3) or None, T_w (S, 4, 4), time (S,), desc (S, d) or None.  The arithmetic follows the
contract term by term (the distance as sqrt((dx^2 + dy^2) + dz^2), the inverse through the cofactors of the 3x3 block, the
products of the 4x4 chain added left to right); only the d-long sums are NumPy's own (their order is free in the contract).

`borderline()` flags an input on which a decision of the gate could depend on the last bits of a sum: generated test inputs
use seeds that carry no flag (`clean_grid` raises on one that does: a flagged seed is a test error, never a skip).
"""
import numpy as np

NEARBY, SKIP, GATED, TODO = 1, 2, 4, 8


def inv_affine(A):
    """(S, 4, 4) affine matrices (bottom row 0 0 0 1) -> their inverses, through the cofactors of the 3x3 block."""
    A = np.asarray(A, dtype=np.float64)
    a, b, c, d, e, f, g, h, i = (A[:, r, k] for r in range(3) for k in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    r = 1.0 / (a * c00 + b * c10 + c * c20)
    I = np.zeros_like(A)
    I[:, 0, 0], I[:, 0, 1], I[:, 0, 2] = c00 * r, c01 * r, c02 * r
    I[:, 1, 0], I[:, 1, 1], I[:, 1, 2] = c10 * r, c11 * r, c12 * r
    I[:, 2, 0], I[:, 2, 1], I[:, 2, 2] = c20 * r, c21 * r, c22 * r
    t = A[:, :3, 3]
    for k in range(3):
        I[:, k, 3] = -(I[:, k, 0] * t[:, 0] + I[:, k, 1] * t[:, 1] + I[:, k, 2] * t[:, 2])
    I[:, 3, 3] = 1.0
    return I


def mul4(A, B):
    """A (S0, 1, 4, 4) times B (1, S1, 4, 4), every entry ((0 + a0 b0) + a1 b1) + ... in that order."""
    C = np.zeros(np.broadcast_shapes(A.shape, B.shape))
    for k in range(4):
        C = C + A[..., :, k, None] * B[..., None, k, :]
    return C


def grid_gate_oracle(side0, side1, radius, skip_distance=np.inf, desc_thresh=0.0, single_robot_lc=False, lc_time_thresh=0.0):
    """-> dict: dist, flags, yaw_deg, sim (S0, S1), T_ij (S0, S1, 4, 4), pairs (n_todo, 2) int32, T_ref (n_todo, 4, 4),
    enable (n_todo,) int32, n_todo, and norm_prod (S0, S1) or None (for borderline())."""
    S0, S1 = len(side0["pos"]), len(side1["pos"])
    gt = side0.get("pos_gt") is not None and side1.get("pos_gt") is not None
    pa = np.asarray(side0["pos_gt"] if gt else side0["pos"], dtype=np.float64).reshape(S0, 3)
    pb = np.asarray(side1["pos_gt"] if gt else side1["pos"], dtype=np.float64).reshape(S1, 3)
    dl = pa[:, None, :] - pb[None, :, :]
    dist = np.sqrt((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2])
    nearby = dist < 2.0 * radius
    T_ij = mul4(inv_affine(np.asarray(side0["T_w"]).reshape(S0, 4, 4))[:, None], np.asarray(side1["T_w"], dtype=np.float64).reshape(S1, 4, 4)[None])
    yaw = np.where(nearby, np.abs(np.arctan2(T_ij[:, :, 1, 0], T_ij[:, :, 0, 0]) * (180.0 / np.pi)), np.nan)
    norm_prod = None
    if side0.get("desc") is None or np.asarray(side0["desc"]).shape[-1] == 0:
        sim = np.full((S0, S1), np.inf)
    else:
        A, Bm = np.asarray(side0["desc"], dtype=np.float64).reshape(S0, -1), np.asarray(side1["desc"], dtype=np.float64).reshape(S1, -1)
        norm_prod = np.sqrt(np.sum(A * A, axis=1))[:, None] * np.sqrt(np.sum(Bm * Bm, axis=1))[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            sim = (A @ Bm.T) / norm_prod
        sim[norm_prod <= 1e-9] = 0.0
    skip = dist > skip_distance
    with np.errstate(invalid="ignore"):
        gated = ~skip & (sim < desc_thresh)
    todo = ~skip & ~gated
    flags = (nearby * NEARBY + skip * SKIP + gated * GATED + todo * TODO).astype(np.int32)
    ti, tj = np.nonzero(todo)
    enable = np.ones(len(ti), dtype=np.int32)
    if single_robot_lc:
        enable[np.abs(np.asarray(side0["time"])[ti] - np.asarray(side1["time"])[tj]) < lc_time_thresh] = 0
    return dict(dist=dist, flags=flags, yaw_deg=yaw, sim=sim, T_ij=T_ij, pairs=np.stack([ti, tj], axis=1).astype(np.int32),
                T_ref=T_ij[ti, tj], enable=enable, n_todo=int(len(ti)), norm_prod=norm_prod)


def borderline(side0, side1, radius, skip_distance=np.inf, desc_thresh=0.0, single_robot_lc=False, lc_time_thresh=0.0):
    """True when a decision sits within rounding of its threshold: dist within 1e-9 of 2 * radius or of skip_distance, sim within
    1e-9 of desc_thresh, |dt| within 1e-9 of lc_time_thresh, a norm product within 1e-12 of 1e-9."""
    o = grid_gate_oracle(side0, side1, radius, skip_distance, desc_thresh, single_robot_lc, lc_time_thresh)
    near = lambda x, t: bool(np.any(np.abs(np.asarray(x) - t) <= 1e-9)) if np.isfinite(t) else False
    if near(o["dist"], 2.0 * radius) or near(o["dist"], skip_distance):
        return True
    if o["norm_prod"] is not None:
        if near(o["sim"][np.isfinite(o["sim"])], desc_thresh) or bool(np.any(np.abs(o["norm_prod"] - 1e-9) <= 1e-12)):
            return True
    if single_robot_lc:
        dt = np.abs(np.asarray(side0["time"])[:, None] - np.asarray(side1["time"])[None, :])
        if near(dt, lc_time_thresh):
            return True
    return False


def yaw_pose(yaw, t):
    T = np.eye(4)
    T[0, 0] = T[1, 1] = np.cos(yaw); T[0, 1] = -np.sin(yaw); T[1, 0] = np.sin(yaw)
    T[:3, 3] = t
    return T


def random_side(rng, S, d, box=30.0, with_gt=False):
    """S gravity-aligned submaps in a box: yaw-only poses at the centres, times over ten minutes, positive-biased descriptors
    (cosines spread over roughly 0.2 ... 0.9)."""
    pos = rng.uniform(-box, box, (S, 3)) * np.array([1.0, 1.0, 0.1])
    T_w = np.array([yaw_pose(rng.uniform(-np.pi, np.pi), pos[s]) for s in range(S)]).reshape(S, 4, 4)
    desc = (rng.normal(0.0, 1.0, (S, d)) + rng.uniform(0.0, 1.5, (S, 1))) if d else None
    return dict(pos=pos, pos_gt=pos + rng.normal(0.0, 0.5, (S, 3)) if with_gt else None, T_w=T_w, time=rng.uniform(0.0, 600.0, S), desc=desc)


def clean_grid(seed, S0, S1, d, gt=(False, False), **gate):
    """The seeded grid for the gate parameters `gate`; a seed that carries a borderline flag is an ERROR (choose another)."""
    rng = np.random.default_rng(seed)
    a, b = random_side(rng, S0, d, with_gt=gt[0]), random_side(rng, S1, d, with_gt=gt[1])
    if S0 and S1 and borderline(a, b, **gate):
        raise AssertionError(f"seed {seed} gives a borderline grid for S0={S0} S1={S1} d={d} {gate}: choose another seed")
    return a, b
