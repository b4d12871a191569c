"""tests/_integrate_oracle.py held to itself and to SciPy, without a GPU: the sort-and-runs down-sample against
the dict-of-accumulators form; the mean neighbour distances against scipy.spatial.cKDTree; the consequences of open3d's outlier
rule at m = 1, 2, 9, 10, 11; and what the planted clouds of tests/test_gpu_segment_integrate.py plant: that the `faces` clouds
tell (p - origin) / vs from (p - origin) * (1 / vs) and a random blob does not, and both sides of the last span the key holds."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _integrate_clouds as clouds
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


def posed(points, seed):
    """`points` taken into the body frame of a random pose and back by the oracle's row-wise expression: a rounding off the faces"""
    T = clouds.pose(seed)
    return io.world_points(clouds.body(points, T), T)


FACE_CLOUDS = {f"faces 600 vs {vs}": (lambda vs=vs: clouds.faces(600, 600, clouds.FACE_CORNER, 12, vs), vs) for vs in clouds.FACE_SIZES}
FACE_CLOUDS.update({f"faces 600 posed vs {vs}": (lambda vs=vs: posed(clouds.faces(600, 600, clouds.FACE_CORNER, 12, vs), 600), vs) for vs in clouds.FACE_SIZES})
FACE_CLOUDS["faces 5000 vs 0.05"] = (lambda: clouds.faces(5000, 5000, clouds.FACE_CORNER, 24, clouds.VS), clouds.VS)


@pytest.mark.parametrize("name", list(FACE_CLOUDS))
def test_face_clouds_tell_the_division_from_a_reciprocal(name):
    """The evidence behind tests/test_gpu_segment_integrate.py::test_keys_planted_on_voxel_faces: on every `faces` cloud of that
    file — as planted, and assembled through a pose — floor((p - origin) * (1 / vs)) differs from floor((p - origin) / vs) in at
    least one row, so a kernel that multiplies by the reciprocal cannot return the oracle's bits there.  The two forms of the
    oracle's down-sample agree on them."""
    make, vs = FACE_CLOUDS[name]
    p = make()
    rows = clouds.cheap_rows(p, vs)
    print(f"{name}: the reciprocal changes the voxel index of {rows} of {len(p)} rows")
    assert rows >= 1
    if "posed" not in name:
        assert np.all(p >= p[0]) and p[0].tolist() == list(clouds.FACE_CORNER)     # the first point is the minimum corner
    a, b = io.down_sample(p, vs), io.down_sample_literal(p, vs)
    assert a.shape == b.shape and a.tobytes() == b.tobytes() and len(a) < len(p)


def test_a_random_blob_does_not_tell_them_apart():
    """... which is why the random clouds alone proved nothing about the division: no quotient of a blob comes near an integer."""
    for seed, n, side in ((5000, 5000, 24.0), (600, 600, 7.0)):
        rows = clouds.cheap_rows(clouds.blob(seed, n, side, clouds.FACE_CORNER), clouds.VS)
        print(f"blob of {n}: the reciprocal changes the voxel index of {rows} rows")
        assert rows == 0


@pytest.mark.parametrize("axes", clouds.SPAN_AXES)
def test_the_last_span_that_fits(axes):
    """Voxel index KEY_TOP = 2^21 - 1 is the last an axis of the key holds; on all three axes the key is 2^63 - 1."""
    vs = clouds.VS
    fits, over = clouds.span_pair(io.KEY_TOP, axes), clouds.span_pair(io.KEY_TOP + 1, axes)
    idx = io.voxel_indices(fits, vs)
    assert idx[0].tolist() == [0, 0, 0] and idx[1].tolist() == [io.KEY_TOP if k in axes else 0 for k in range(3)]
    if len(axes) == 3:
        assert int(io.pack(idx)[1]) == 2 ** 63 - 1
    assert io.down_sample(fits, vs).tobytes() == fits.tobytes() == io.down_sample_literal(fits, vs).tobytes()
    r = io.cleanup(fits, io.params(vs, None))
    assert r.status == io.OK and len(r.points) == 2
    assert io.voxel_indices(over, vs) is None and io.down_sample(over, vs) is None
    r = io.cleanup(over, io.params(vs, 1.0))
    assert r.status == io.RANGE and len(r.points) == 0 and r.avg is None
    # padded with 300 points in the positive octant the minimum corner, and so both answers, stay
    seed = 40 + clouds.SPAN_AXES.index(axes)
    for t, status in ((io.KEY_TOP, io.OK), (io.KEY_TOP + 1, io.RANGE)):
        p = clouds.span_padded(seed, t, axes)
        assert np.all(p.min(axis=0) == 0.0) and io.cleanup(p, io.params(vs, None)).status == status
    p = clouds.span_padded(seed, io.KEY_TOP, axes)
    idx = io.voxel_indices(p, vs)
    far = np.all(idx == idx[1], axis=1)
    assert far.sum() == 1 and (len(axes) < 3 or np.argmax(io.pack(idx)) == 1)


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
