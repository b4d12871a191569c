"""The two forms of tests/_voxel_oracle.py against each other, no GPU: the SET form the device computes — global
keys, a count inside [lo, hi) — equals the LITERAL form, the reference's dense arrays and slices, on random and planted clouds."""
import numpy as np
import pytest

import _voxel_oracle as vo

SIZES = (0.2, 0.05, 1.0, 0.1, 0.37)


def random_cloud(rng, vs, centre, on_faces):
    n = int(rng.integers(1, 201))
    p = centre + rng.normal(size=(n, 3)) * rng.uniform(0.2, 6.0) * vs
    if on_faces:                                            # points exactly on multiples of the voxel size
        k = rng.random(n) < 0.5
        p[k] = np.round(p[k] / vs) * vs
    return p


def both_forms(a, b, vs):
    ga, gb = vo.literal_grid(a, vs), vo.literal_grid(b, vs)
    ra, rb = vo.cloud_record(a, vs), vo.cloud_record(b, vs)
    assert ra.status == rb.status == vo.OK
    assert ra.n_vox == int(np.sum(ga.voxels)) and rb.n_vox == int(np.sum(gb.voxels))
    inter = vo.set_intersection(ra, rb)
    lit = vo.literal_intersection(ga, gb)
    assert lit == inter * vs**3, (lit, inter)
    for method, iom in ((vo.IOU, False), (vo.IOM, True)):
        want = vo.literal_iou(ga, gb, iom_as_iou=iom)
        got = vo.geo_from_counts(ra.n_vox, rb.n_vox, inter, vs, method)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (method, got, want)
    return inter, ra, rb


def truncation_quirk(rec, vs):
    """A corner whose truncated integer is not the rounded one: floor(x / vs) * vs / vs fell just off an integer."""
    return bool(np.any(rec.mci != np.rint(rec.minc / vs)) or np.any(rec.maxci != np.rint(rec.maxc / vs)))


def test_set_form_equals_literal_form_on_random_pairs():
    rng = np.random.default_rng(20250)
    nonzero = quirks = 0
    for it in range(4000):
        vs = SIZES[it % len(SIZES)]
        centre = rng.uniform(-3.0, 3.0, 3) * (1.0 if it % 3 else 40.0) * vs * 5     # negative coordinates, straddling zero
        a = random_cloud(rng, vs, centre, it % 4 == 0)
        b = random_cloud(rng, vs, centre + rng.normal(size=3) * rng.uniform(0.0, 4.0) * vs, it % 4 == 1)
        inter, ra, rb = both_forms(a, b, vs)
        nonzero += inter > 0
        quirks += truncation_quirk(ra, vs) or truncation_quirk(rb, vs)
    assert nonzero > 1000 and quirks > 0, (nonzero, quirks)


def planted():
    vs = 0.2
    c = (np.arange(4) + 0.5) * vs
    cube = np.array([[x, y, z] for x in c for y in c for z in c])             # 64 voxels, every point in its own
    yield "identical", cube, cube, vs
    yield "nested", cube, cube[:8], vs
    yield "touching", cube, cube + np.array([4 * vs, 0.0, 0.0]), vs
    yield "one voxel", np.tile(c[:1], (50, 3)), np.tile(c[:1], (7, 3)) + 0.01, vs
    yield "straddling zero", cube - 2 * vs, cube - 2.5 * vs, vs
    yield "on the faces", np.round(cube / vs) * vs, np.round(cube / vs) * vs - vs, vs
    yield "overlap without a common voxel", np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.7]]), vs
    for vs in (0.05, 1.0):
        yield f"scaled {vs}", cube / 0.2 * vs, cube[::3] / 0.2 * vs + 0.4 * vs, vs


@pytest.mark.parametrize("case", list(planted()), ids=lambda c: c[0])
def test_planted_cases(case):
    name, a, b, vs = case
    inter, ra, rb = both_forms(a, b, vs)
    if name == "identical":
        assert vo.geo_from_counts(ra.n_vox, rb.n_vox, inter, vs, vo.IOU) == 1.0
    if name == "nested":
        assert vo.geo_from_counts(ra.n_vox, rb.n_vox, inter, vs, vo.IOM) == 1.0 and inter == rb.n_vox
    if name in ("touching", "overlap without a common voxel"):
        assert inter == 0


def test_a_shared_key_in_the_padding_layer_counts_in_the_volume_only():
    """A point on the top face of its cloud's box lands, by the half-voxel shift, in a voxel outside [min_corner_int,
    max_corner_int): it is a voxel of the volume and can never be part of an intersection, in either form."""
    vs = 0.2
    a = np.array([[0.1, 0.1, 0.1], [0.3, 0.3, 0.4]])        # z = 0.4 is a multiple of vs: max_corner_int z = 2, the point's key z = 2
    ra = vo.cloud_record(a, vs)
    pad = vo.padding_keys(ra)
    assert len(pad) == 1
    b = np.array([[0.1, 0.1, 0.1], [0.3, 0.3, 0.45], [0.5, 0.5, 0.9]])
    rb = vo.cloud_record(b, vs)
    shared = {tuple(k) for k in ra.keys.tolist()} & {tuple(k) for k in rb.keys.tolist()}
    assert tuple(pad[0].tolist()) in shared
    inter, _, _ = both_forms(a, b, vs)
    assert inter == len(shared) - 1


def test_empty_and_out_of_range_clouds_have_no_voxel():
    p = vo.params()
    far = np.array([[3.0e5, 0.0, 0.0], [3.0e5 + 0.1, 0.1, 0.1]])            # 1.5e6 voxels of 0.2 from the origin: more than 2^20
    near = np.array([[0.1, 0.1, 0.1]])
    r = vo.scores([near, np.zeros((0, 3)), far, np.array([[np.nan, 0.0, 0.0]])], [near], p)
    assert r.status.tolist() == [vo.OK, vo.EMPTY, vo.RANGE, vo.RANGE, vo.OK] and r.n_vox.tolist() == [1, 0, 0, 0, 1]
    assert r.geo[:, 0].tolist() == [1.0, 0.0, 0.0, 0.0] and r.score[:, 0].tolist() == [-1.0, vo.M, vo.M, vo.M]
    edge = np.array([[(vo.KEY_BIAS - 2) * 0.2 + 0.05, 0.0, 0.0]])
    assert vo.cloud_record(edge, 0.2).status == vo.OK and vo.cloud_record(edge + np.array([0.4, 0, 0]), 0.2).status == vo.RANGE


def test_score_rule():
    p1, p2 = vo.params(), vo.params(semantic=True)
    assert vo.score_of(0.25, None, p1) == -0.25 and vo.score_of(np.nextafter(0.25, 0), None, p1) == vo.M
    assert vo.score_of(0.5, 0.79, p2) == vo.M and vo.score_of(0.2, 0.9, p2) == vo.M
    want = -np.power(((0.5 - 0.25) / 0.75) * ((0.9 - 0.8) / (1.0 - 0.8)), 0.5)
    assert vo.score_of(0.5, 0.9, p2) == want
    assert np.isnan(vo.score_of(0.5, np.nan, p2))                         # NaN is not < lo: it propagates
    assert vo.cosine(None, np.ones(3)) == 1.0 and np.isnan(vo.cosine(np.zeros(3), np.ones(3)))
    assert vo.gnn_pairs(np.array([[-0.9, vo.M], [vo.M, vo.M]])) == [(0, 0)]
