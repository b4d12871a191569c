"""tests/_integrate_oracle.py held to itself and to SciPy, without a GPU: the sort-and-runs down-sample against
the dict-of-accumulators form; the mean neighbour distances against scipy.spatial.cKDTree; the consequences of open3d's outlier
rule at m = 1, 2, 9, 10, 11."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _integrate_oracle as io

VOXEL_SIZES = (0.05, 0.1, 0.2, 0.3, 1.0)


def cloud(seed, n, vs):
    """A random cloud around a negative centre with repeated points and points exactly on voxel faces."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)) * (4.0 * vs) + np.array([-3.0, 0.5, -0.25])
    p[::7] = np.round(p[::7] / vs) * vs                    # on voxel faces of a grid through 0
    p[::11] = p[0]
    p[1::13, 1] = p[-1, 1]
    return p


@pytest.mark.parametrize("vs", VOXEL_SIZES)
@pytest.mark.parametrize("seed,n", [(0, 1), (1, 2), (2, 37), (3, 400), (4, 1500)])
def test_down_sample_agrees_with_the_literal_form(seed, n, vs):
    p = cloud(seed, n, vs)
    a, b = io.down_sample(p, vs), io.down_sample_literal(p, vs)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert 1 <= len(a) <= n
    # the points on the faces: shifted to put the minimum itself on a face, so that (p - origin) / vs sits at k + 0.5 exactly
    q = np.round(p / vs) * vs
    a, b = io.down_sample(q, vs), io.down_sample_literal(q, vs)
    assert a.tobytes() == b.tobytes()
    assert len(a) == len(np.unique(io.pack(io.voxel_indices(q, vs))))


def test_down_sample_order_and_range():
    vs = 0.5
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 1.0], [2.1, 0.1, 0.0]])
    d = io.down_sample(p, vs)
    # ascending key, x most significant: the voxel of (0, 0, 0), of (0, 0, 1), of (2, 0, 0)
    assert d.tolist() == [[(0.0 + 0.1) / 2.0, 0.0, 0.0], [0.0, 0.0, 1.0], [(2.0 + 2.1) / 2.0, (0.0 + 0.1) / 2.0, 0.0]]
    assert io.down_sample(np.array([[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]]), vs) is None
    assert io.down_sample(np.array([[0.0, 0.0, np.nan]]), vs) is None
    assert io.down_sample(np.array([[0.0, 0.0, 0.0], [vs * 2.0 ** 21, 0.0, 0.0]]), vs) is None
    assert len(io.down_sample(np.array([[0.0, 0.0, 0.0], [vs * (2.0 ** 21 - 2), 0.0, 0.0]]), vs)) == 2


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("seed,m", [(0, 1), (1, 2), (2, 9), (3, 10), (4, 11), (5, 300), (6, 1200)])
def test_mean_neighbor_distances_agree_with_ckdtree(seed, m):
    pts = np.random.default_rng(seed).normal(size=(m, 3))
    k = min(10, m)
    d, _ = cKDTree(pts).query(pts, k=k)
    ref = np.asarray(d).reshape(m, k).mean(axis=1)
    avg = io.mean_neighbor_distances(pts)
    assert avg.shape == (m,)
    nz = ref > 0
    assert np.array_equal(avg == 0, ~nz)
    assert np.all(ulps(avg[nz], ref[nz]) <= 4), ulps(avg[nz], ref[nz]).max()


def test_world_points_is_the_rowwise_expression():
    rng = np.random.default_rng(5)
    T = np.eye(4); T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]; T[:3, 3] = [1.0, -2.0, 0.5]
    p = rng.normal(size=(50, 3))
    w = io.world_points(p, T)
    assert np.allclose(w, p @ T[:3, :3].T + T[:3, 3], rtol=0, atol=1e-14)
    assert w[7, 1] == ((T[1, 0] * p[7, 0] + T[1, 1] * p[7, 1]) + T[1, 2] * p[7, 2]) + T[1, 3]
    assert io.world_points(p, None).tobytes() == p.tobytes()


def spaced(m):
    """m points far apart on a line, one per voxel, with unequal gaps"""
    return np.stack([np.cumsum(1.0 + 0.1 * np.arange(m)), np.zeros(m), np.zeros(m)], axis=1)


def test_planted_small_clouds():
    P = io.params(0.05, 1.0)
    r = io.cleanup(spaced(1), P)                           # m = 1: avg = 0, m - 1 = 0 gives a NaN threshold, nothing is kept
    assert len(r.down) == 1 and r.avg.tolist() == [0.0] and np.isnan(r.thr) and len(r.points) == 0 and r.status == io.OK
    r = io.cleanup(spaced(2), P)                           # m = 2: equal avg, std = 0, x < x is false
    assert len(r.down) == 2 and r.avg[0] == r.avg[1] > 0 and r.thr == r.avg[0] and len(r.points) == 0
    for m in (9, 10, 11):
        r = io.cleanup(spaced(m), P)
        k = min(10, m)
        d = np.abs(r.down[:, None, 0] - r.down[None, :, 0])
        ref = np.sort(d, axis=1)[:, :k].mean(axis=1)
        assert len(r.down) == m and np.allclose(r.avg, ref, rtol=1e-15, atol=0)
        keep = (r.avg > 0) & (r.avg < r.thr)
        assert 0 < keep.sum() < m and r.points.tobytes() == r.down[keep].tobytes()
    # m = 11 is the first size at which a point does not reach every other one
    r = io.cleanup(spaced(11), P)
    assert r.avg[0] < np.abs(r.down[:, 0] - r.down[0, 0]).sum() / 10.0


def test_outlier_step_off_and_the_empty_added_cloud():
    p = cloud(9, 200, 0.1)
    for std in (None, 0.0, -1.0, np.inf):
        r = io.cleanup(p, io.params(0.1, std))
        assert r.avg is None and r.thr is None and r.points.tobytes() == io.down_sample(p, 0.1).tobytes()
    P = io.params(0.1, 1.0)
    r = io.integrate(p, np.zeros((0, 3)), None, P)         # _add_points' early return: no clean-up
    assert r.points.tobytes() == p.tobytes() and r.status == io.OK
    assert io.integrate(None, np.zeros((0, 3)), None, P).status == io.EMPTY
    a = io.integrate(None, p, None, P)
    b = io.integrate(np.zeros((0, 3)), p, None, P)
    assert a.points.tobytes() == b.points.tobytes() == io.cleanup(p, P).points.tobytes()


@pytest.mark.parametrize("m", [2, 3, 64, 65, 1000, 5000])
def test_threshold_in_fixed_order_lies_inside_its_bound(m):
    avg = np.abs(np.random.default_rng(m).normal(size=m)) + 0.01
    avg[::17] = 0.0
    assert io.fixed_sum(avg) == io.fixed_sum(avg) and abs(io.fixed_sum(avg) - avg.sum()) <= io.sum_depth(m) * 2.0 ** -53 * avg.sum()
    thr = io.threshold(avg, 1.0)
    truth, bound = io.threshold_truth(avg, 1.0)
    assert abs(thr - truth) <= bound and bound < 1e-13 * truth
