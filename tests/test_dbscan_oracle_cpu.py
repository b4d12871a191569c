"""tests/_dbscan_oracle.py on its own (no device): open3d's sequential loop, stated literally, equals the closed
form the kernels implement; core flags and the core partition agree with scikit-learn's DBSCAN where no distance sits on the
radius; and every planted cloud of tests/_cluster_clouds.py has the property it is planted for."""
import numpy as np
import pytest

import _cluster_clouds as cc
import _dbscan_oracle as do
from _cluster_clouds import EPS, MIN_POINTS


def random_cloud(rng, k):
    n = int(rng.integers(1, 120))
    p = rng.uniform(0.0, rng.uniform(0.4, 1.6), (n, 3))
    if k % 3 == 0:
        p = np.round(p / 0.05) * 0.05          # many equal distances, some of them on a radius
    return p


def test_sequential_loop_equals_closed_form():
    rng = np.random.default_rng(27)
    kinds = {"multi": 0, "single": 0, "noise": 0}
    runs = 0
    for k in range(240):
        p = random_cloud(rng, k)
        for mp in (1, 3, 5, 10):
            eps = (0.15, 0.25, 0.4)[(k + mp) % 3]
            seq, closed = do.labels_sequential(p, eps, mp), do.labels_closed(p, eps, mp)
            assert np.array_equal(seq, closed), (k, mp, eps)
            nc = int(closed.max()) + 1
            kinds["multi" if nc > 1 else "single" if nc == 1 else "noise"] += 1
            runs += 1
    print(kinds)
    assert min(kinds.values()) >= runs // 20, f"the sample is one-sided: {kinds}"


def partition(labels, mask):
    """the sets of indices that share a label, over the points of `mask`"""
    return {frozenset(np.flatnonzero((labels == l) & mask).tolist()) for l in set(labels[mask].tolist())}


def test_core_points_and_partition_agree_with_sklearn():
    import sklearn.cluster as sk
    done = 0
    for seed in range(12):
        p = cc.clumps(100 + seed, (90, 200, 400)[seed % 3])
        for eps, mp in ((EPS, MIN_POINTS), (0.15, 5), (0.4, 3)):
            assert do.edge_gap_ulps(p, eps) > 4.0, "a distance within 4 ulp of the radius: sklearn's comparison is inclusive"
            ref = sk.DBSCAN(eps=eps, min_samples=mp, algorithm="brute").fit(p)
            core = do.core_flags(p, eps, mp)
            ref_core = np.zeros(len(p), dtype=bool)
            ref_core[ref.core_sample_indices_] = True
            assert np.array_equal(core, ref_core), (seed, eps, mp)
            lab = do.labels_closed(p, eps, mp)
            assert partition(lab, core) == partition(ref.labels_, core), (seed, eps, mp)
            assert np.array_equal(lab == -1, ref.labels_ == -1), (seed, eps, mp)
            done += int(core.any())
    assert done >= 24


def test_shared_border_point():
    for order in ("last", "first", "swapped", "interleaved"):
        p, x, a, b = cc.shared_border(order)
        nb, core = do.neighbours(p, EPS), do.core_flags(p, EPS, MIN_POINTS)
        lab = do.labels_closed(p, EPS, MIN_POINTS)
        assert np.array_equal(lab, do.labels_sequential(p, EPS, MIN_POINTS))
        assert not core[x] and core[a].all() and core[b].all() and nb[x].sum() == 5
        assert len(set(lab[a])) == 1 and len(set(lab[b])) == 1 and lab[a[0]] != lab[b[0]], "two clusters"
        assert (nb[x] & core)[a].any() and (nb[x] & core)[b].any(), "X has core neighbours in both clusters"
        assert lab[x] == 0 == min(lab[a[0]], lab[b[0]])
        assert (lab[b[0]] == 0) == (order in ("swapped", "interleaved"))
    p, x, a, b = cc.shared_border("first")
    assert x == 0                                                   # the sequential loop meets it first: noise, then relabelled
    p, x, a, b = cc.shared_border("interleaved")
    assert b[0] == 0 and b[1] > a.max()


def test_size_tie_and_border_decides():
    r = do.final_cleanup(cc.size_tie(), EPS)
    assert r.n_clusters == 2 and r.kept == 0 and len(r.points) == 15 and np.sum(r.labels == 1) == 15
    p = cc.border_decides()
    r = do.final_cleanup(p, EPS)
    core = do.core_flags(p, EPS, MIN_POINTS)
    assert r.n_clusters == 2 and core.sum() == 30 and not core[30] and r.labels[30] == 1
    assert r.kept == 1 and len(r.points) == 16 and r.points.tobytes() == p[15:].tobytes()


def test_chains_are_one_deep_component():
    for p in (cc.chain(600, True)[0], cc.chain(600, False)[0], cc.chain(1100, False)[0], cc.u_chain()):
        lab = do.labels_closed(p, EPS, 3)
        assert np.all(lab == 0) and do.core_flags(p, EPS, 3).all() and do.neighbours(p, EPS).sum(axis=1).max() <= 6   # a line, and the corner of the U
    p, pos = cc.chain(600, True)
    assert pos[0] == 300 and not np.array_equal(pos, np.arange(600))
    u = cc.u_chain()
    nb = do.neighbours(u, EPS)
    assert not nb[:300, 300:600].any(), "the arms touch only through the rung"
    assert nb[299, 600:].any() and nb[599, 600:].any()


def test_radius_edge():
    p = cc.radius_lattice()
    e2 = do.d2_matrix(p)
    assert np.sum(e2 == 0.25 * 0.25) == 2 * 54, "every lattice edge sits exactly on the radius"
    at, above = do.labels_closed(p, 0.25, 2), do.labels_closed(p, np.nextafter(0.25, 1.0), 2)
    assert np.all(at == -1) and np.all(above == 0) and not np.array_equal(at, above)
    assert np.array_equal(do.labels_closed(p, 0.25, 1), np.arange(27))
    assert np.array_equal(at, do.labels_sequential(p, 0.25, 2)) and np.array_equal(above, do.labels_sequential(p, np.nextafter(0.25, 1.0), 2))


def test_small_and_degenerate():
    r = do.final_cleanup(cc.duplicates(10), EPS)
    assert r.n_clusters == 1 and len(r.points) == 10 and np.all(r.labels == 0)
    r = do.final_cleanup(cc.duplicates(9), EPS)
    assert r.status == do.OK and r.n_clusters == 0 and r.kept == -1 and len(r.points) == 0
    r = do.final_cleanup(np.array([[1.0, 2.0, 3.0]]), EPS, 1)
    assert r.n_clusters == 1 and r.kept == 0 and len(r.points) == 1
    r = do.final_cleanup(cc.sparse(50), EPS)
    assert r.n_clusters == 0 and np.all(r.labels == -1) and len(r.points) == 0
    assert do.final_cleanup(np.zeros((0, 3)), EPS).status == do.EMPTY
    bad = cc.clumps(1, 40)
    bad[7, 1] = np.nan
    assert do.final_cleanup(bad, EPS).status == do.RANGE
    bad[7, 1] = np.inf
    assert do.final_cleanup(bad, EPS).status == do.RANGE


def test_clumps_hold_clusters_borders_and_noise():
    for n in (255, 600, 1537):
        p = cc.clumps(n, n)
        r = do.final_cleanup(p, EPS)
        core = do.core_flags(p, EPS, MIN_POINTS)
        assert r.n_clusters >= 2 and np.any(r.labels == -1) and np.any((r.labels >= 0) & ~core), n
        assert np.array_equal(r.labels, do.labels_sequential(p, EPS, MIN_POINTS)), n
