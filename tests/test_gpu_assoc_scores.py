"""Frame data association scores through the C ABI: roman_assoc_scores* against tests/_voxel_oracle.py.

n_vox, inter and status are EXACT and geo is BIT FOR BIT in both methods: the device forms integer counts and then runs the
oracle's f64 operations in the oracle's order.  score is bit for bit where it is 1e9 or -geo.

THE TOLERANCES of the cosine are derived, not measured.  The device's dot product over d terms is a sum of depth at most
ceil(d / 64) - 1 + 6 with one rounding per product, so on descriptors of norm <= 1 its error is below (d + 1) 2^-53; the two norms
carry (d + 2) 2^-53 relative each, the product of the norms and the division one rounding each: together below (d + 4) 2^-52
absolute for |cos| <= 1, the standard bound.  The truth is formed in longdouble.  In two-criterion mode the score is compared
with the oracle's formula evaluated ON THE DEVICE'S geo and sem: the formula's own four operations agree bit for bit, the square
root is correctly rounded on the device and np.power(x, 0.5) is within 1 ulp of that: 2 ulp."""
import ctypes as C

import numpy as np
import pytest

import _voxel_oracle as vo
from _hipmem import Hip
from conftest import ulp_diff
from roman_amd import _abi
from roman_amd.align import SegmentClouds
from roman_amd.map import AssociationParams, association_scores, global_nearest_neighbor
from roman_amd.runtime import assoc_params

pytestmark = pytest.mark.gpu

W, L = _abi.ROMAN_ASSOC_WAVE_MAX, _abi.ROMAN_ASSOC_LDS_MAX
GUARD = -7.25e300


def pack(clouds):
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    if clouds:
        off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.vstack([np.zeros((0, 3))] + [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]))
    return pts, off


def abi_of(p):
    return assoc_params(p.voxel_size, p.geometric, p.semantic, p.geo_range, p.sem_range)


def run(ctx, rows, cols, p, desc=None, **kw):
    pts, off = pack(rows + (cols or []))
    return ctx.assoc_scores(abi_of(p), pts, off, len(rows), -1 if cols is None else len(cols), desc, **kw)


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def check(ctx, rows, cols, p, desc=None):
    """One call against the oracle: counts and status exact, geo bit for bit; one criterion: score bit for bit."""
    got = run(ctx, rows, cols, p, desc)
    n1 = len(rows)
    want = vo.scores(rows, cols, p, None if desc is None else desc[:n1], None if desc is None or cols is None else desc[n1:])
    if want.geo.size == 0:                                  # no pair: ROMAN_OK with nothing written, the per-cloud outputs included
        assert not got.status.any() and not got.n_vox.any() and got.geo.shape == want.geo.shape
        return got, want
    assert np.array_equal(got.status, want.status), (got.status, want.status)
    assert np.array_equal(got.n_vox, want.n_vox), (got.n_vox, want.n_vox)
    assert np.array_equal(got.inter, want.inter)
    assert same_bits(got.geo, want.geo)
    if not p.semantic:
        assert got.sem is None and same_bits(got.score, want.score)
    return got, want


def blob(rng, n, vs, centre=(0.0, 0.0, 0.0), radius=7.0):
    """n points uniform in a cube of 2 * radius voxels a side (a long cloud fills every voxel many times over)."""
    return np.asarray(centre) + rng.uniform(-radius, radius, (n, 3)) * vs


def lattice(n, vs, origin=(0.0, 0.0, 0.0)):
    """n points, every one alone in its voxel (centres of the first n cells of a 32-wide lattice)."""
    i = np.arange(n)
    return np.asarray(origin) + (np.stack([i % 32, (i // 32) % 32, i // 1024], axis=1) + 0.5) * vs


# ------------------------------------------------------------------------------------------------------------ sizes and paths
@pytest.mark.parametrize("vs", [0.2, 0.05, 1.0])
@pytest.mark.parametrize("method", ["iou", "iom"])
def test_cloud_sizes_on_every_path(ctx, vs, method):
    """1, 2, 63, 64, 65 points, one point either side of both path cuts, and a cloud of several merge passes: as random blobs
    (many points per voxel) and as lattices (every point in its own voxel), against two columns that overlap them."""
    rng = np.random.default_rng(5)
    sizes = [1, 2, 63, 64, 65, W - 1, W, W + 1, L - 1, L, L + 1, 4 * L + 77]
    rows = [blob(rng, n, vs, radius=9.0) if k % 2 == 0 else lattice(n, vs, (-8 * vs, -8 * vs, -3 * vs)) for k, n in enumerate(sizes)]
    rows.append(np.tile([[0.31 * vs, -0.2 * vs, 0.4 * vs]], (300, 1)))                      # all points in one voxel
    cols = [blob(rng, 900, vs, radius=6.0), lattice(1500, vs, (-8 * vs, -8 * vs, -3 * vs))]
    got, want = check(ctx, rows, cols, vo.params(vs, method, geo_range=(0.05, 1.0)))
    assert want.n_vox[1] == 2 and want.n_vox[10] < sizes[10] and want.n_vox[12] == 1 and want.n_vox[9] == L and want.n_vox[11] == sizes[11]   # duplicates, and none
    assert np.count_nonzero(want.inter) >= 20 and np.any(want.score == vo.M) and np.any(want.score < 0)


def test_results_do_not_depend_on_the_cuts(ctx):
    """With the cuts lowered to 16 and 64 points, clouds of a few thousand points take up to six merge passes and clouds of 17 to
    64 points the LDS workgroup: the same answer as with the default cuts, and the oracle's."""
    rng = np.random.default_rng(6)
    sizes = [3, 16, 17, 64, 65, 127, 128, 129, 1000, 2048, 2049, 4000]
    rows = [blob(rng, n, 0.2, radius=8.0) for n in sizes]
    p = vo.params(0.2, "iou")
    base, _ = check(ctx, rows, None, p)
    ctx.set_assoc_cuts(16, 64)
    try:
        low, _ = check(ctx, rows, None, p)
    finally:
        ctx.set_assoc_cuts(0, 0)
    assert np.array_equal(base.inter, low.inter) and same_bits(base.score, low.score)
    with pytest.raises(_abi.RomanHipError):
        ctx.set_assoc_cuts(600, 0)


@pytest.mark.parametrize("n1,n2", [(1, 1), (3, 5), (65, 2), (0, 4), (4, 0), (5, -1)])
def test_grid_shapes_and_self_mode(ctx, n1, n2):
    rng = np.random.default_rng(n1 * 10 + n2 + 1)
    rows = [blob(rng, int(rng.integers(1, 90)), 0.2, rng.normal(size=3) * 0.3, radius=3.0) for _ in range(n1)]
    cols = None if n2 < 0 else [blob(rng, int(rng.integers(1, 90)), 0.2, rng.normal(size=3) * 0.3, radius=3.0) for _ in range(n2)]
    got, want = check(ctx, rows, cols, vo.params(0.2, "iou", geo_range=(0.1, 1.0)))
    assert got.geo.shape == (n1, n1 if n2 < 0 else n2)
    if n2 < 0:                                              # every ordered pair is computed; the reference's IoU and IoM are symmetric
        assert same_bits(got.geo, got.geo.T) and np.array_equal(got.inter, got.inter.T)
        assert np.all(np.diag(got.inter) <= got.n_vox) and np.all(np.diag(got.inter) > 0)   # (a padding-layer voxel is outside even a cloud's own intersection)
        iom, _ = check(ctx, rows, None, vo.params(0.2, "iom"))
        assert same_bits(iom.geo, iom.geo.T)


# ------------------------------------------------------------------------------------------------------------ planted coordinates
def truncation_case():
    """A corner whose float falls just below its integer: floor(x / vs) * vs / vs truncates to one less (searched on the CPU)."""
    for vs in (0.2, 0.05):
        for k in range(1, 4000):
            x = (k + 0.25) * vs
            c = np.floor(x / vs) * vs
            if int(c / vs) != int(np.floor(x / vs)):
                return vs, k, x
    return None


@pytest.mark.parametrize("vs", [0.2, 0.05, 1.0])
def test_coordinate_cases(ctx, vs):
    rng = np.random.default_rng(8)
    straddle = [blob(rng, 200, vs, radius=2.5), blob(rng, 150, vs, (0.3 * vs, -0.6 * vs, 0.2 * vs), radius=2.5), blob(rng, 40, vs, (-vs, -vs, -vs), radius=1.0)]
    on_faces = [np.round(c / vs) * vs for c in straddle] + [np.round(straddle[0] / vs) * vs - vs]
    for method in ("iou", "iom"):
        _, want = check(ctx, straddle + on_faces, None, vo.params(vs, method))
        assert np.count_nonzero(want.inter) > 30
        assert any(np.any(vo.cloud_record(c, vs).mci < 0) and np.any(vo.cloud_record(c, vs).maxci > 0) for c in straddle)


def test_the_truncation_quirk_is_planted_and_followed(ctx):
    found = truncation_case()
    assert found is not None, "no corner of the searched range truncates below its integer"
    vs, k, x = found
    rng = np.random.default_rng(9)
    a = np.array([x, 0.1 * vs, 0.1 * vs]) + rng.uniform(0, 3, (60, 3)) * vs
    a[0] = [x, 0.1 * vs, 0.1 * vs]                          # the minimum of the first axis sits on the planted coordinate
    b = a[::2] + np.array([0.0, 0.5 * vs, 0.0])
    ra = vo.cloud_record(a, vs)
    assert ra.mci[0] == k - 1 and np.rint(ra.minc[0] / vs) == k
    for method in ("iou", "iom"):
        check(ctx, [a, b], [b, a], vo.params(vs, method))


def test_box_cases(ctx):
    vs = 0.2
    c = (np.arange(4) + 0.5) * vs
    cube = np.array([[x, y, z] for x in c for y in c for z in c])
    touching = cube + np.array([4 * vs, 0.0, 0.0])
    sparse_a, sparse_b = np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.7]])
    pad_a = np.array([[0.1, 0.1, 0.1], [0.3, 0.3, 0.4]])
    pad_b = np.array([[0.1, 0.1, 0.1], [0.3, 0.3, 0.45], [0.5, 0.5, 0.9]])
    rows = [cube, cube[:8], sparse_a, pad_a]
    cols = [cube, touching, cube[:8], sparse_b, pad_b]
    iou, w = check(ctx, rows, cols, vo.params(vs, "iou"))
    iom, _ = check(ctx, rows, cols, vo.params(vs, "iom"))
    assert iou.geo[0, 0] == 1.0 and iou.inter[0, 0] == 64                                  # identical clouds
    assert iou.inter[0, 1] == 0 and iou.geo[0, 1] == 0.0 and iou.score[0, 1] == vo.M        # boxes that touch: min == max
    ra, rb = vo.cloud_record(cube, vs), vo.cloud_record(touching, vs)
    assert np.any(np.maximum(ra.minc, rb.minc) == np.minimum(ra.maxc, rb.maxc))
    assert iom.geo[0, 2] == 1.0 and iou.geo[0, 2] == 8 / 64 and iou.geo[1, 0] == 8 / 64    # nested: IoM 1, IoU a / b
    assert iou.inter[2, 3] == 0 and np.all(np.maximum(vo.cloud_record(sparse_a, vs).minc, vo.cloud_record(sparse_b, vs).minc)
                                           < np.minimum(vo.cloud_record(sparse_a, vs).maxc, vo.cloud_record(sparse_b, vs).maxc))   # overlapping boxes, no common voxel
    pa, pb = vo.cloud_record(pad_a, vs), vo.cloud_record(pad_b, vs)
    shared = {tuple(k) for k in pa.keys.tolist()} & {tuple(k) for k in pb.keys.tolist()}
    pad = vo.padding_keys(pa)
    assert len(pad) == 1 and tuple(pad[0].tolist()) in shared                               # a shared key in a padding layer ...
    assert iou.inter[3, 4] == len(shared) - 1 and iou.n_vox[3] == 2                         # ... counts in the volume, not in the intersection


def test_planted_thresholds_decide_exactly(ctx):
    """1 of 4 voxels: IoU 0.25.  The threshold exactly at the similarity, one ulp above it and one ulp below."""
    for vs in (1.0, 0.2):
        a, b = lattice(1, vs), lattice(4, vs)
        g = vo.geo_from_counts(1, 4, 1, vs, vo.IOU)
        if vs == 1.0:
            assert g == 0.25
        for lo, passes in ((g, True), (np.nextafter(g, 1.0), False), (np.nextafter(g, 0.0), True)):
            got, _ = check(ctx, [a], [b], vo.params(vs, "iou", geo_range=(lo, 1.0)))
            assert same_bits(got.geo[0, 0], g) and same_bits(got.score[0, 0], -g if passes else vo.M)
            d = np.array([[2.0, 0.0, 0.0], [4.0, 0.0, 0.0]])                               # cosine exactly 1.0
            for slo, sem_passes in ((1.0, True), (np.nextafter(1.0, 2.0), False), (np.nextafter(1.0, 0.0), True)):
                p2 = vo.params(vs, "iou", True, (lo, 1.0), (slo, 2.0))
                got2 = run(ctx, [a], [b], p2, d)
                assert got2.sem[0, 0] == 1.0
                want = vo.score_of(g, 1.0, p2) if passes and sem_passes else vo.M
                assert (got2.score[0, 0] == vo.M) == (want == vo.M) and ulp_diff(got2.score[0, 0], want) <= 2


# ------------------------------------------------------------------------------------------------------------ other clouds
def test_empty_and_out_of_range_clouds(ctx):
    vs = 0.2
    near = lattice(5, vs)
    far = np.array([[3.0e5, 0.0, 0.0], [3.0e5 + 0.1, 0.1, 0.1]])
    nan = np.array([[0.1, np.nan, 0.1], [0.1, 0.1, 0.1]])
    edge_in = np.array([[(vo.KEY_BIAS - 2) * vs + 0.05, 0.0, 0.0]])
    rows, cols = [near, np.zeros((0, 3)), far, nan, edge_in, edge_in + np.array([0.4, 0, 0])], [np.zeros((0, 3)), near, far]
    for method in ("iou", "iom"):
        got, want = check(ctx, rows, cols, vo.params(vs, method))
        assert got.status.tolist() == [0, vo.EMPTY, vo.RANGE, vo.RANGE, 0, vo.RANGE, vo.EMPTY, 0, vo.RANGE]
        assert got.n_vox.tolist() == [5, 0, 0, 0, 1, 0, 0, 5, 0]
        assert got.geo[0, 1] == 1.0 and np.count_nonzero(got.geo) == 1 and np.count_nonzero(got.score != vo.M) == 1


@pytest.mark.parametrize("d", [0, 1, 16, 769])
def test_cosine_and_the_two_criterion_score(ctx, d):
    rng = np.random.default_rng(d + 3)
    vs, n1, n2 = 0.2, 4, 3
    rows = [blob(rng, 80, vs, radius=2.0) for _ in range(n1)]
    cols = [rows[j % n1][::2] + 0.01 for j in range(n2)] + [rows[0]]
    n2 += 1
    desc = None
    if d:
        desc = rng.normal(size=(n1 + n2, d))
        desc[n1:] = desc[np.arange(n2) % n1] + 0.3 * rng.normal(size=(n2, d)) * (d > 1)
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        desc[n1 + n2 - 1] = 0.0                                                            # a zero descriptor: 0 / 0, NaN propagates
    p = vo.params(vs, "iou", True, (0.05, 1.0), (0.5, 1.0))
    got, want = check(ctx, rows, cols, p, desc)
    assert got.geo[0, n2 - 1] > 0.25                       # the same cloud on both sides (short of 1.0 by its padding-layer voxels)
    if d == 0:                                             # no descriptors: the cosine of every pair is 1.0
        assert np.all(got.sem == 1.0)
    else:
        ld = desc.astype(np.longdouble)
        with np.errstate(all="ignore"):
            truth = (ld[:n1] @ ld[n1:].T) / np.outer(np.sqrt((ld[:n1]**2).sum(1)), np.sqrt((ld[n1:]**2).sum(1)))
        err = np.abs(got.sem[:, :-1].astype(np.longdouble) - truth[:, :-1]).max()
        print(f"d = {d}: cosine error {float(err):.3e}, bound {(d + 4) * 2.0**-52:.3e}")
        assert err <= (d + 4) * 2.0**-52
        assert np.all(np.isnan(got.sem[:, -1])) and np.isnan(got.score[0, -1])             # geo passes, the NaN is not below its threshold
    for i in range(n1):
        for j in range(n2):
            w = vo.score_of(got.geo[i, j], got.sem[i, j], p)
            if np.isnan(w) or w == vo.M:
                assert same_bits(got.score[i, j], w) or (np.isnan(w) and np.isnan(got.score[i, j]))
            else:
                assert ulp_diff(got.score[i, j], w) <= 2 and same_bits(got.score[i, j], vo.score_of(got.geo[i, j], got.sem[i, j], p, sqrt=True))
    assert np.any(got.score < 0) and (d < 16 or np.any(got.score == vo.M))


# ------------------------------------------------------------------------------------------------------------ general
def test_determinism_forms_optional_outputs_and_capacity(ctx):
    rng = np.random.default_rng(12)
    vs = 0.2
    rows = [blob(rng, n, vs, radius=4.0) for n in (50, 300, 700)]
    cols = [blob(rng, n, vs, radius=4.0) for n in (40, 600)]
    desc = rng.normal(size=(5, 16))
    p = vo.params(vs, "iou", True, (0.05, 1.0), (-1.0, 1.0))
    a, b = run(ctx, rows, cols, p, desc), run(ctx, rows, cols, p, desc)
    for f in ("geo", "sem", "score", "inter", "n_vox", "status"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    # NULL optional outputs
    c = run(ctx, rows, cols, p, desc, want_sem=False, want_inter=False, want_n_vox=False)
    assert c.sem is None and c.inter is None and c.n_vox is None and same_bits(c.score, a.score) and same_bits(c.geo, a.geo)
    # the device form, with capacity behind every output
    hip = Hip()
    try:
        pts, off = pack(rows + cols)
        extra, pairs, clouds = 7, 6, 5
        f64 = lambda n: hip.upload(np.full(n + extra, GUARD))
        i32 = lambda n: hip.upload(np.full(n + extra, -77, dtype=np.int32))
        d_geo, d_sem, d_score, d_inter, d_nv, d_st = f64(pairs), f64(pairs), f64(pairs), i32(pairs), i32(clouds), i32(clouds)
        ctx.assoc_scores_dev(abi_of(p), hip.upload(pts), hip.upload(off), off, 3, 2, hip.upload(desc), 16, d_geo, d_score, d_st,
                             sem_ptr=d_sem, inter_ptr=d_inter, n_vox_ptr=d_nv)
        ctx.sync()
        for ptr, n, dt, want, guard in ((d_geo, pairs, np.float64, a.geo, GUARD), (d_sem, pairs, np.float64, a.sem, GUARD), (d_score, pairs, np.float64, a.score, GUARD),
                                        (d_inter, pairs, np.int32, a.inter, -77), (d_nv, clouds, np.int32, a.n_vox, -77), (d_st, clouds, np.int32, a.status, -77)):
            out = hip.download(ptr, n + extra, dt)
            assert out[:n].tobytes() == want.tobytes() and np.all(out[n:] == guard)
        # semantic = 0 leaves sem untouched
        p1 = vo.params(vs, "iou", False, (0.05, 1.0))
        ctx.assoc_scores_dev(abi_of(p1), hip.upload(pts), hip.upload(off), off, 3, 2, None, 0, d_geo, d_score, d_st, sem_ptr=d_sem)
        ctx.sync()
        assert hip.download(d_sem, pairs, np.float64).tobytes() == a.sem.tobytes()
    finally:
        hip.free_all()
    # a second call with other sizes on the same context
    check(ctx, cols + rows[:1], rows[1:], vo.params(0.05, "iom"))
    check(ctx, rows[:1], None, vo.params(1.0, "iou"))


# ------------------------------------------------------------------------------------------------------------ the association
def clouds_of(list_of_points, desc=None):
    pts, off = pack(list_of_points)
    n = len(list_of_points)
    return SegmentClouds(pts, off, np.arange(n, dtype=np.int64), np.zeros((n, 2)), desc)


def test_global_nearest_neighbor_returns_the_oracles_pairs(ctx):
    """Scenes whose optimum is unique by construction: row i is a lattice block of its own, far from the others; a column is the
    first m_j cells of one row's block, so its IoU with that row is m_j / 64 — distinct values, one candidate per row and column —
    and exactly 0 with every other row."""
    vs = 0.2
    block = lambda i: lattice(64, vs, (10.0 * i, -3.0, 1.0))
    rows = [block(i) for i in range(5)]
    part = lambda i, m: block(i)[:m]
    P = AssociationParams()
    scenes = {
        "mixed": [part(3, 60), part(0, 40), part(1, 10), part(4, 17), lattice(30, vs, (-50.0, 0.0, 0.0))],    # 10 / 64 is below the threshold
        "all matched": [part(4, 64), part(2, 33), part(0, 50), part(1, 20), part(3, 41)],
        "all unmatched": [lattice(20, vs, (-50.0 - 10 * j, 0.0, 0.0)) for j in range(3)],
    }
    want = {"mixed": [(0, 1), (3, 0), (4, 3)], "all matched": [(0, 2), (1, 3), (2, 1), (3, 4), (4, 0)], "all unmatched": []}
    for name, cols in scenes.items():
        r = association_scores(clouds_of(rows), clouds_of(cols), P, ctx=ctx)
        o = vo.scores(rows, cols, vo.params())
        assert same_bits(r.score, o.score) and np.array_equal(r.inter, o.inter) and r.sem is None
        live = o.score[o.score != vo.M]
        assert len(np.unique(live)) == len(live) and np.all(np.count_nonzero(o.score != vo.M, axis=0) <= 1) and np.all(np.count_nonzero(o.score != vo.M, axis=1) <= 1)
        pairs = global_nearest_neighbor(clouds_of(rows), clouds_of(cols), P, ctx=ctx)
        assert pairs == vo.gnn_pairs(o.score) == want[name], name
    # self mode, as merge() compares the segments, and the two-criterion path through the Python layer
    rng = np.random.default_rng(4)
    desc = rng.normal(size=(5, 16))
    P2 = AssociationParams(geometric_association_method="iom", semantic_association_method="cosine_similarity", semantic_score_range=(0.5, 1.0))
    s = association_scores(clouds_of(rows + [part(2, 30)], np.vstack([desc, desc[2:3]])), None, P2, ctx=ctx)
    assert s.geo.shape == (6, 6) and s.geo[2, 5] == 1.0 and s.geo[5, 2] == 1.0 and abs(s.sem[2, 5] - 1.0) <= 20 * 2.0**-52
    assert s.score[2, 5] != vo.M and s.score[0, 1] == vo.M
