"""The planted clouds of the segment update's tests, shared by tests/test_gpu_segment_integrate.py and
tests/test_integrate_oracle_cpu.py.  No device code — TEST INFRASTRUCTURE."""
import numpy as np

import _integrate_oracle as io

VS = 0.05
FACE_CORNER = (3.0, -1.0, 0.5)
FACE_SIZES = (0.05, 0.2, 0.03)            # voxel sizes of the 600-point face clouds
SPAN_AXES = ((0, 1, 2), (0,), (1,), (2,))  # the axes a two-point cloud spans: all three at once, and each alone


def blob(seed, n, side, centre=(0.0, 0.0, 0.0)):
    """n points uniform in a cube of `side` voxels"""
    return np.asarray(centre) + np.random.default_rng(seed).uniform(-0.5 * side, 0.5 * side, (n, 3)) * VS


def lattice(seed, n, origin=(0.0, 0.0, 0.0)):
    """n points, every one alone in its voxel: cell centres of a 7-wide lattice with gaps, jittered by a fifth of a voxel"""
    i = np.arange(n)
    cells = np.stack([i % 7, (i // 7) % 7, i // 49], axis=1) * np.array([1.0, 2.0, 1.0])
    return np.asarray(origin) + (cells + 0.5 + np.random.default_rng(seed).uniform(-0.2, 0.2, (n, 3))) * VS


def pose(seed):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T[:3, :3] = q * np.sign(np.linalg.det(q))
    T[:3, 3] = rng.normal(size=3)
    return T


def body(points, T):
    """the points in the body frame of pose T (so that the posed cloud lands where `points` is, up to rounding)"""
    return (np.asarray(points) - T[:3, 3]) @ T[:3, :3]


def faces(seed, n, corner, span, vs):
    """n points ON voxel faces: the first is `corner` itself — the minimum on every axis, so the origin is corner - vs / 2 — and
    the others are corner + (k + 0.5) vs with integer k in [0, span) per axis.  (p - origin) / vs is then k + 1 up to its
    roundings, and floor() of it depends on every one of them."""
    k = np.random.default_rng(seed).integers(0, span, (n, 3)).astype(np.float64)
    p = np.asarray(corner, dtype=np.float64) + (k + 0.5) * vs
    p[0] = corner
    return p


def cheap_indices(points, vs):
    """io.voxel_indices with the division replaced by a multiplication with the rounded reciprocal: what the tests must tell apart"""
    origin = np.min(points, axis=0) - 0.5 * vs
    return np.floor((points - origin) * (1.0 / vs)).astype(np.int64)


def cheap_rows(points, vs):
    """rows of `points` whose voxel index differs between the division and the reciprocal"""
    return int(np.sum(np.any(io.voxel_indices(points, vs) != cheap_indices(points, vs), axis=1)))


def span_pair(t, axes, vs=VS):
    """(0, 0, 0) and a point whose voxel index on `axes` is t: the origin is -vs / 2, so vs (t - 0.5) sits in the middle of voxel t"""
    p = np.zeros((2, 3))
    p[1, list(axes)] = vs * (t - 0.5)
    return p


def span_padded(seed, t, axes, vs=VS):
    """span_pair and 300 points of a blob in the positive octant next to the first corner: the minimum stays (0, 0, 0)"""
    return np.concatenate([span_pair(t, axes, vs), blob(seed, 300, 6.0, (0.2, 0.2, 0.2))], axis=0)
