"""roman_segment_cluster on the device against tests/_dbscan_oracle.py.

Every output is an integer or a copied double: labels, n_clusters, kept, count, status and the kept points are the oracle's BIT
FOR BIT; there is no tolerance in this file.  Every case runs through the device-pointer form into arrays that carry a sentinel
in front of the first slot, behind the last one and in every element: what a job does not write — its slot of out_points past
out_count, the labels of an EMPTY or RANGE job, the guard rows — must still hold it.  Every case runs twice (identical bytes) and
under three cut settings, so that each job is taken by one wave, by the workgroup that holds it in LDS and by the tiled class
through global memory: identical bytes again.  The planted clouds are tests/_cluster_clouds.py's; tests/test_dbscan_oracle_cpu.py
shows on the oracle that each has the property it is planted for."""
from types import SimpleNamespace

import numpy as np
import pytest

import _cluster_clouds as cc
import _dbscan_oracle as do
from _cluster_clouds import EPS, MIN_POINTS
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.align import SegmentClouds, SubmapAlignParams
from roman_amd.align.submaps import MapTable
from roman_amd.map import ClusterParams, cluster_labels, final_cleanup, retire
from roman_amd.runtime import cluster_params, cluster_slots

pytestmark = pytest.mark.gpu

GUARD, LGUARD, IGUARD, PAD = -7.25e300, -77, -55, 8
WAVE, LDS, TILE, COLS = _abi.ROMAN_CLUSTER_WAVE_MAX, _abi.ROMAN_CLUSTER_LDS_MAX, _abi.ROMAN_CLUSTER_TILE, _abi.ROMAN_CLUSTER_COLS
# default: one wave up to 256, LDS workgroup up to 1536, tiled beyond | low: one wave up to 16, LDS up to 64, tiled from 65 on |
# mid: one wave up to 32, the LDS workgroup for everything else it can hold
CUTS = {"default": (0, 0), "low": (16, 64), "mid": (32, LDS)}


def case(name, clouds, eps=EPS, mp=MIN_POINTS, jobs=None):
    return SimpleNamespace(name=name, clouds=clouds, eps=eps, mp=mp, jobs=list(range(len(clouds))) if jobs is None else jobs)


def poisoned(seed, n, value, row=7):
    p = cc.clumps(seed, n)
    p[row, 1] = value
    return p


def make_cases():
    edges_low = (15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1)
    edges_default = (WAVE - 1, WAVE, WAVE + 1, COLS - 1, COLS, COLS + 1, LDS - 1, LDS, LDS + 1)
    return {c.name: c for c in (
        case("border", [cc.shared_border(o)[0] for o in ("last", "first", "swapped", "interleaved")] + [cc.size_tie(), cc.border_decides()]),
        case("chains", [cc.chain(600, True)[0], cc.u_chain(), cc.chain(600, False)[0], cc.chain(1100, False)[0]], mp=3),
        case("radius_at", [cc.radius_lattice()], eps=0.25, mp=2),
        case("radius_above", [cc.radius_lattice()], eps=float(np.nextafter(0.25, 1.0)), mp=2),
        case("radius_singletons", [cc.radius_lattice(), cc.radius_lattice(5)], eps=0.25, mp=1),
        case("small", [cc.duplicates(10), cc.duplicates(9), cc.sparse(50), np.zeros((0, 3)), cc.clumps(3, 90), poisoned(4, 80, np.nan), cc.clumps(5, 70),
                       poisoned(6, 300, np.inf, 299), cc.clumps(7, 120), poisoned(8, 1600, -np.inf, 1599), cc.clumps(9, 40)]),
        case("single", [np.array([[1.0, 2.0, 3.0]]), np.zeros((0, 3)), np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [5.0, 0.0, 0.0]])], mp=1),
        case("edges_low", [cc.clumps(n, n, snap=n % 2 == 0) for n in edges_low]),
        case("edges_default", [cc.clumps(n, n) for n in edges_default]),
        case("mixed", [cc.clumps(21, 2000), cc.clumps(22, 100), cc.clumps(23, 600, snap=True)]),
        case("sparse_jobs", [cc.clumps(30 + k, n) for k, n in enumerate((50, 0, 70, 300, 20, 90, 40))], jobs=[5, 0, 3]),
    )}


CASES = make_cases()
_ORACLE = {}


def oracle(name):
    """The oracle's answer per job of a case, computed once."""
    if name not in _ORACLE:
        c = CASES[name]
        _ORACLE[name] = [do.final_cleanup(c.clouds[k], c.eps, c.mp) for k in c.jobs]
    return _ORACLE[name]


def pack(clouds):
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.ascontiguousarray(np.vstack([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds])), off


def run(ctx, c, cuts="default", labels=True):
    """One call of the device form; every output lies inside a larger array full of sentinels -> the arrays, guards included."""
    hip = Hip()
    pts, off = pack(c.clouds)
    jobs = np.asarray(c.jobs, dtype=np.int32)
    nj, total = len(jobs), int(cluster_slots(off, jobs)[-1])
    d_pts, d_off, d_jobs = hip.upload(pts), hip.upload(off), hip.upload(jobs)
    o_pts = hip.upload(np.full((total + 2 * PAD, 3), GUARD))
    o_lab = hip.upload(np.full(total + 2 * PAD, LGUARD, dtype=np.int32))
    o_int = hip.upload(np.full((4, nj + 2 * PAD), IGUARD, dtype=np.int32))                 # count, status, n_clusters, kept
    row = lambda k: o_int + 4 * (k * (nj + 2 * PAD) + PAD)                                 # behind the guard in front
    ctx.set_cluster_cuts(*CUTS[cuts])
    try:
        ctx.segment_cluster_dev(cluster_params(c.eps, c.mp), d_pts, d_off, off, d_jobs, jobs, o_pts + 24 * PAD, row(0), row(1), row(2),
                                out_labels_ptr=o_lab + 4 * PAD if labels else None, out_kept_ptr=row(3))
        ctx.sync()
        return SimpleNamespace(points=hip.download(o_pts, (total + 2 * PAD, 3), np.float64), label=hip.download(o_lab, (total + 2 * PAD,), np.int32),
                               ints=hip.download(o_int, (4, nj + 2 * PAD), np.int32), slot=cluster_slots(off, jobs), n_jobs=nj)
    finally:
        ctx.set_cluster_cuts(0, 0)
        hip.free_all()


def same(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("points", "label", "ints"))


def check(c, out, labels=True):
    """bit for bit against the oracle; everything a job does not write still holds its sentinel"""
    ref = oracle(c.name)
    nj, total = out.n_jobs, int(out.slot[-1])
    assert np.all(out.points[:PAD] == GUARD) and np.all(out.points[PAD + total:] == GUARD), (c.name, "a write in front of or behind out_points")
    assert np.all(out.label[:PAD] == LGUARD) and np.all(out.label[PAD + total:] == LGUARD), (c.name, "a write in front of or behind out_labels")
    assert np.all(out.ints[:, :PAD] == IGUARD) and np.all(out.ints[:, PAD + nj:] == IGUARD), (c.name, "a write in front of or behind a per-job output")
    count, status, n_clusters, kept = (out.ints[k, PAD:PAD + nj] for k in range(4))
    for j, r in enumerate(ref):
        s0, s1 = PAD + out.slot[j], PAD + out.slot[j + 1]
        tag = (c.name, j)
        assert status[j] == r.status and n_clusters[j] == r.n_clusters and kept[j] == r.kept and count[j] == len(r.points), tag
        assert out.points[s0:s0 + count[j]].tobytes() == r.points.tobytes(), tag
        assert np.all(out.points[s0 + count[j]:s1] == GUARD), (tag, "the slot past out_count was written")
        if labels and r.labels is not None:
            assert out.label[s0:s1].tobytes() == r.labels.tobytes(), (tag, np.flatnonzero(out.label[s0:s1] != r.labels)[:8])
        else:
            assert np.all(out.label[s0:s1] == LGUARD), (tag, "labels written for an EMPTY / RANGE job or without out_labels")


def through_every_class(ctx, c):
    first = run(ctx, c)
    check(c, first)
    assert same(first, run(ctx, c)), (c.name, "two calls differ")
    for cuts in ("low", "mid"):
        assert same(first, run(ctx, c, cuts)), (c.name, f"the cuts {cuts} = {CUTS[cuts]} give other bytes")
    return first


# ----------------------------------------------------------------------------------------------------------------- the tests
def test_shared_border_size_tie_and_the_border_point_that_decides(ctx):
    out = through_every_class(ctx, CASES["border"])
    kept = out.ints[3, PAD:PAD + 6]
    assert kept.tolist() == [0, 0, 0, 0, 0, 1]
    for j, order in enumerate(("last", "first", "swapped", "interleaved")):
        _, x, a, b = cc.shared_border(order)
        lab = out.label[PAD + out.slot[j]:PAD + out.slot[j + 1]]
        assert lab[x] == 0 and lab[b[0]] == (0 if order in ("swapped", "interleaved") else 1) and lab[a[0]] == 1 - lab[b[0]]


def test_depth_of_the_union(ctx):
    """Chains as deep as the cloud: 600 shuffled points with index 0 mid-chain, a U that joins at the far end, and chains in
    index order that cross every query tile (256) and the column staging (1024) of the tiled class under the low cuts."""
    c = CASES["chains"]
    assert [len(p) for p in c.clouds] == [600, 609, 600, 1100] and 600 > 2 * TILE and 1100 > COLS and CUTS["low"][1] < 600
    out = through_every_class(ctx, c)
    assert out.ints[2, PAD:PAD + 4].tolist() == [1, 1, 1, 1] and out.ints[0, PAD:PAD + 4].tolist() == [600, 609, 600, 1100]


def test_radius_edge(ctx):
    at, above = oracle("radius_at")[0], oracle("radius_above")[0]
    assert not np.array_equal(at.labels, above.labels) and at.n_clusters == 0 and above.n_clusters == 1
    through_every_class(ctx, CASES["radius_at"])
    through_every_class(ctx, CASES["radius_above"])
    out = through_every_class(ctx, CASES["radius_singletons"])
    assert out.ints[2, PAD:PAD + 2].tolist() == [27, 125] and out.ints[0, PAD:PAD + 2].tolist() == [1, 1] and out.ints[3, PAD:PAD + 2].tolist() == [0, 0]


def test_small_and_degenerate(ctx):
    """Ten duplicates (one cluster), nine (none), 50 sparse points (all noise), an empty cloud, a NaN, +Inf and -Inf coordinate in a
    wave-class, an LDS-class and a tiled-class job with untouched neighbours in between; then n = 1 with min_points = 1."""
    c = CASES["small"]
    out = through_every_class(ctx, c)
    status = out.ints[1, PAD:PAD + len(c.jobs)].tolist()
    assert status == [do.OK, do.OK, do.OK, do.EMPTY, do.OK, do.RANGE, do.OK, do.RANGE, do.OK, do.RANGE, do.OK]
    assert out.ints[0, PAD:PAD + 4].tolist() == [10, 0, 0, 0] and out.ints[3, PAD + 1:PAD + 4].tolist() == [-1, -1, -1]
    assert [len(c.clouds[k]) for k in (5, 7, 9)] == [80, 300, 1600] and 80 <= WAVE < 300 <= LDS < 1600
    one = through_every_class(ctx, CASES["single"])
    assert one.ints[0, PAD:PAD + 3].tolist() == [1, 0, 2] and one.ints[2, PAD:PAD + 3].tolist() == [1, 0, 2]


@pytest.mark.parametrize("name", ["edges_low", "edges_default", "mixed"])
def test_staging_and_class_edges(ctx, name):
    """n = cut - 1, cut, cut + 1 of both class boundaries at the lowered cuts (16, 64) and at the default ones (256, 1536); n around
    the query tile (256) and the column staging (1024) of the tiled class; one call mixing a job of each class."""
    c = CASES[name]
    n = [len(c.clouds[k]) for k in c.jobs]
    if name == "mixed":
        assert n[0] > LDS and n[1] <= WAVE and WAVE < n[2] <= LDS
    else:
        assert all(m - 1 in n and m + 1 in n for m in ((16, 64, TILE) if name == "edges_low" else (WAVE, COLS, LDS)))
    through_every_class(ctx, c)
    assert any(r.n_clusters >= 2 for r in oracle(name)) and any(np.any(r.labels == -1) for r in oracle(name))


def test_sparse_job_list_without_labels_and_the_host_form(ctx):
    """Jobs name clouds 5, 0, 3 of 7: slots in job order, the other clouds never read into an output.  Without out_labels the
    labels stay in the workspace.  The host-pointer form returns the same bytes and leaves what a job does not write as it was."""
    c = CASES["sparse_jobs"]
    out = through_every_class(ctx, c)
    assert out.slot.tolist() == [0, 90, 140, 440]
    bare = run(ctx, c, labels=False)
    check(c, bare, labels=False)
    assert bare.points.tobytes() == out.points.tobytes() and bare.ints.tobytes() == out.ints.tobytes()
    pts, off = pack(c.clouds)
    host = ctx.segment_cluster(cluster_params(c.eps, c.mp), pts, off, c.jobs, out_points=np.full((440, 3), GUARD), out_labels=np.full(440, LGUARD, np.int32))
    assert host.points.tobytes() == out.points[PAD:-PAD].tobytes() and host.label.tobytes() == out.label[PAD:-PAD].tobytes()
    assert np.stack([host.count, host.status, host.n_clusters, host.kept]).tobytes() == np.ascontiguousarray(out.ints[:, PAD:-PAD]).tobytes()
    for j, r in enumerate(oracle(c.name)):
        assert host.cloud(j).tobytes() == r.points.tobytes() and host.labels(j).tobytes() == r.labels.tobytes()


def test_no_job_is_ok_and_writes_nothing(ctx):
    import ctypes as C
    pts, off = pack([cc.clumps(1, 20), cc.clumps(2, 30)])
    P = cluster_params()
    out_points, ints, lab = np.full((50, 3), GUARD), np.full((4, 2), IGUARD, np.int32), np.full(50, LGUARD, np.int32)
    jobs = np.array([1], dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib, h = ctx._lib, ctx._h
    assert lib.roman_segment_cluster(h, C.byref(P), p(pts), p(off), 2, p(jobs), 0, p(out_points), p(ints[0]), p(ints[1]), p(lab), p(ints[2]), p(ints[3])) == _abi.ROMAN_OK
    assert lib.roman_segment_cluster(h, C.byref(P), p(pts), p(off), 2, None, 0, None, None, None, None, None, None) == _abi.ROMAN_OK
    # the device form returns behind the argument checks, before any device pointer is looked at
    assert lib.roman_segment_cluster_dev(h, C.byref(P), p(pts), None, p(off), 2, None, None, 0, None, None, None, None, None, None) == _abi.ROMAN_OK
    ctx.sync()
    assert np.all(out_points == GUARD) and np.all(ints == IGUARD) and np.all(lab == LGUARD)
    r = ctx.segment_cluster(P, pts, off, [])
    assert r.points.shape == (0, 3) and r.count.shape == (0,) and r.label.shape == (0,) and r.slot.tolist() == [0]
    e = ctx.segment_cluster(P, np.zeros((0, 3)), np.zeros(3, np.int64), [1, 0])      # every slot is empty: no out_points to give
    assert e.count.tolist() == [0, 0] and e.status.tolist() == [do.EMPTY, do.EMPTY] and e.n_clusters.tolist() == [0, 0] and e.kept.tolist() == [-1, -1]


def test_the_cuts_hook_refuses_what_the_lds_cannot_hold(ctx):
    from roman_amd._abi import RomanHipError
    for bad in ((WAVE + 1, 0), (0, LDS + 1), (-1, 0), (65, 64)):
        with pytest.raises(RomanHipError):
            ctx.set_cluster_cuts(*bad)
    ctx.set_cluster_cuts(0, 0)


def test_final_cleanup_and_retire_end_to_end(ctx):
    """A scripted map at t = 20: segment 0 (two clusters of 15 and 20 points and three noise points, last seen at 2) and segment 1
    (all noise, last seen at 3) have not been seen for more than 10; segment 2 holds no point; segment 3 was seen at 15 and stays.
    The inactive clouds go through MapTable.from_point_clouds: the rows equal those of the oracle-cleaned clouds."""
    D = 8
    rng = np.random.default_rng(5)
    two = np.vstack([cc.rod(0.0, -1, 15), [[9.0, 9.0, 9.0]], cc.rod(5.0, 1, 20), [[-9.0, 3.0, 0.0], [4.0, -7.0, 2.0]]])
    clouds = [two, cc.sparse(30), np.zeros((0, 3)), cc.clumps(40, 200)]
    pts, off = pack(clouds)
    S = SegmentClouds(pts, off, np.array([11, 22, 33, 44]), np.array([[1.0, 2.0], [1.0, 3.0], [1.0, 19.0], [5.0, 15.0]]), rng.normal(size=(4, D)))
    P = ClusterParams.from_mapper_params(SimpleNamespace(clustering_epsilon=EPS))
    ref = do.final_cleanup(two, EPS)
    assert ref.n_clusters == 2 and ref.kept == 1 and len(ref.points) == 20 and np.sum(ref.labels == -1) == 3

    res = final_cleanup(S, [1, 0], P, ctx=ctx)
    assert res.dropped.tolist() == [1] and res.n_clusters.tolist() == [0, 2] and res.kept.tolist() == [-1, 1] and res.status.tolist() == [do.OK, do.OK]
    assert res.clouds.seg_off.tolist() == [0, 0, 20] and res.clouds.points.tobytes() == ref.points.tobytes()
    assert res.clouds.ids.tolist() == [22, 11] and res.clouds.times.tobytes() == S.times[[1, 0]].tobytes() and res.clouds.descriptors.tobytes() == S.descriptors[[1, 0]].tobytes()
    assert cluster_labels(two, P, ctx=ctx).tobytes() == ref.labels.tobytes()

    active, inactive, dropped = retire(S, 20.0, None, 10.0, P, ctx=ctx)
    assert active.tolist() == [3] and sorted(dropped.tolist()) == [22, 33]
    assert inactive.ids.tolist() == [11] and inactive.seg_off.tolist() == [0, 20] and inactive.points.tobytes() == ref.points.tobytes()
    assert inactive.times.tobytes() == S.times[:1].tobytes() and inactive.descriptors.tobytes() == S.descriptors[:1].tobytes()
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    reg.set_context(ctx)
    want = SegmentClouds(ref.points, np.array([0, 20], dtype=np.int64), np.array([11]), S.times[:1], S.descriptors[:1])
    got_t, want_t = MapTable.from_point_clouds(reg, inactive, ctx=ctx), MapTable.from_point_clouds(reg, want, ctx=ctx)
    assert got_t.feats.tobytes() == want_t.feats.tobytes() and got_t.ids.tobytes() == want_t.ids.tobytes() and got_t.times.tobytes() == want_t.times.tobytes()
    dirty = MapTable.from_point_clouds(reg, SegmentClouds(two, np.array([0, len(two)], dtype=np.int64), np.array([11]), S.times[:1], S.descriptors[:1]), ctx=ctx)
    assert dirty.feats[0, :3].tobytes() != got_t.feats[0, :3].tobytes(), "the pre-clustering cloud has another centre: the clean-up is not a no-op here"
