"""The planted clouds of the segment-clustering tests — TEST INFRASTRUCTURE.  Every cloud is generated from a seed
or a closed formula; tests/test_dbscan_oracle_cpu.py asserts on the oracle that each has the property it is planted for."""
import numpy as np

EPS = 0.25                                 # MapperParams.clustering_epsilon [REF roman/params/mapper_params.py:68]
MIN_POINTS = 10                            # final_cleanup's default [REF roman/object/segment.py:195]
STEP = 0.02                                # spacing of a `rod`: a point sees the 12 next ones on either side


def rod(x0, direction, n=15, y=0.0, z=0.0):
    """n points from x0 on, STEP apart along +x (direction 1) or -x (-1).  n >= 10 within 0.25: every point is a core point at
    MIN_POINTS = 10, and a point 0.22 beyond the rod's head sees only the head and the next one."""
    k = np.arange(n, dtype=np.float64)
    return np.stack([x0 + direction * STEP * k, np.full(n, y), np.full(n, z)], axis=1)


def shared_border(order):
    """Rods A (head at x = 0, towards -x) and B (head at x = 0.44, towards +x): 0.44 apart, no link.  X = (0.22, 0, 0) is within eps
    of two points of each and of nothing else: 5 neighbours, not a core point, a border point of BOTH clusters.
      'last'         A, B, X        X takes A's label 0
      'first'        X, A, B        the sequential loop marks X noise first and relabels it
      'swapped'      B, A, X        B holds the lower label now
      'interleaved'  B[0], A, B[1:], X   the lower label belongs to the rod whose bulk is stored later
    -> (points, index of X, indices of A, indices of B)"""
    A, B, X = rod(0.0, -1), rod(0.44, 1), np.array([[0.22, 0.0, 0.0]])
    parts = {"last": [("A", A), ("B", B), ("X", X)], "first": [("X", X), ("A", A), ("B", B)], "swapped": [("B", B), ("A", A), ("X", X)],
             "interleaved": [("B", B[:1]), ("A", A), ("B", B[1:]), ("X", X)]}[order]
    pts = np.vstack([p for _, p in parts])
    who = np.concatenate([[name] * len(p) for name, p in parts])
    return pts, int(np.flatnonzero(who == "X")[0]), np.flatnonzero(who == "A"), np.flatnonzero(who == "B")


def size_tie():
    """two rods far apart, 15 points each: equal sizes, the lower label is kept"""
    return np.vstack([rod(0.0, -1), rod(5.0, 1)])


def border_decides():
    """Two rods of 15 core points each; the second has one border point 0.22 beyond its head: 16 > 15, label 1 is kept."""
    return np.vstack([rod(0.0, -1), rod(5.0, 1), [[5.0 - 0.22, 0.0, 0.0]]])


def chain(n, shuffle, seed=0):
    """n points 0.1 apart on a line: with eps 0.25 and min_points 3 every point is a core point and sees two on either side — one
    component whose union-find is as deep as the chain.  shuffle: a random order in which index 0 sits mid-chain."""
    pos = np.arange(n)
    if shuffle:
        pos = np.random.default_rng(seed).permutation(n)
        k = int(np.flatnonzero(pos == n // 2)[0])
        pos[[0, k]] = pos[[k, 0]]
    return np.stack([0.1 * pos, np.zeros(n), np.zeros(n)], axis=1), pos


def u_chain(arm=300):
    """Two parallel chains 1.0 apart, both indexed from their open end, joined only at the far end by a rung of 9 points."""
    t = 0.1 * np.arange(arm)
    a = np.stack([t, np.zeros(arm), np.zeros(arm)], axis=1)
    b = np.stack([t, np.ones(arm), np.zeros(arm)], axis=1)
    rung = np.stack([np.full(9, t[-1]), 0.1 * np.arange(1, 10), np.zeros(9)], axis=1)
    return np.vstack([a, b, rung])


def radius_lattice(side=3):
    """side^3 points exactly 0.25 apart (multiples of 0.25 are exact): d2 of lattice neighbours == 0.25 * 0.25 exactly."""
    g = 0.25 * np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def duplicates(n=10):
    return np.tile(np.array([[0.3, -1.2, 2.5]]), (n, 1))


def sparse(n=50):
    """n points 1.0 apart: all noise"""
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], axis=1)


def clumps(seed, n, snap=False):
    """n points: four fifths in Gaussian clumps (sigma 0.12) of about 60 points, a fifth uniform in the box that holds the clumps'
    centres — clusters of different sizes, border points and noise at eps 0.25, min_points 10.  snap: coordinates rounded to a
    lattice of 0.05, which plants many equal distances."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 60)
    side = 1.5 * k ** (1.0 / 3.0)
    centres = rng.uniform(0.0, side, (k, 3))
    inside = rng.uniform(size=n) < 0.8
    p = np.where(inside[:, None], centres[rng.integers(0, k, n)] + rng.normal(0.0, 0.12, (n, 3)), rng.uniform(0.0, side, (n, 3)))
    if snap:
        p = np.round(p / 0.05) * 0.05
    return np.ascontiguousarray(p)
