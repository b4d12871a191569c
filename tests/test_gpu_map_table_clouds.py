"""MapTable.from_point_clouds on the device against MapTable.from_segments over MinimalSegments that hold the
ORACLE's values (tests/_segment_shapes_oracle.py): a synthetic map of 60 segments, roman_amd.synth.make_map's centres with clouds of
5 ... 300 points scattered around them here.  Descriptor columns, times and ids: byte for byte.  Shape columns: within the bounds
derived in tests/test_gpu_segment_shapes.py.  With center_ref='bottom_middle' and a RansacReg the rows hold centres only and the
centre is a selection: that table, and the submap pool built from it, equal the oracle's BYTE FOR BYTE.  In 'mean' mode with
method='roman', submap_align_pools over pools from the device table and from the oracle table makes the same decisions."""
import numpy as np
import pytest

import _segment_shapes_oracle as so
from roman_amd import _abi, synth
from roman_amd.align import MinimalSegment, RansacReg, SegmentClouds, SubmapAlignParams
from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers

pytestmark = pytest.mark.gpu
D = 16


@pytest.fixture(scope="module")
def world():
    """-> (clouds, per-segment point arrays, trajectory, times)"""
    segs, trajectory, times = synth.make_map(60, D, seed=8300)
    rng = np.random.default_rng(8301)
    for s in segs:
        n = int(rng.integers(5, 301))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        s.points = (rng.uniform(-0.5, 0.5, (n, 3)) * (0.3, 1.1, 2.7) * rng.uniform(0.5, 1.5)) @ q.T + np.asarray(s.center).reshape(-1)[:3]
    return SegmentClouds.from_segments(segs), [s.points for s in segs], trajectory, times


def oracle_segments(clouds, pts, center_ref="mean"):
    out = []
    for i, p in enumerate(pts):
        o = so.segment(p, center_ref)
        out.append(MinimalSegment(clouds.ids[i], o["center"], o["volume"], *o["ratios"], o["extent"], clouds.descriptors[i], *clouds.times[i]))
    return out


def registrations():
    return {"roman": SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(),
            "sevg": SubmapAlignParams(method="sevg", semantics_dim=D).get_object_registration(),
            "prune-on-device": SubmapAlignParams(method="clipper+prune").get_object_registration().on_device(D),
            "ransac": RansacReg()}


@pytest.mark.parametrize("name", ["roman", "sevg", "prune-on-device", "ransac"])
def test_device_table_against_oracle_table(ctx, world, name):
    clouds, pts, _, _ = world
    reg = registrations()[name]
    reg.set_context(ctx)
    got = MapTable.from_point_clouds(reg, clouds, ctx=ctx)
    want = MapTable.from_segments(reg, oracle_segments(clouds, pts))
    assert got.feats.shape == want.feats.shape
    assert (got.point_dim, got.desc_dim, got.invariant) == (want.point_dim, want.desc_dim, want.invariant)
    assert got.times.tobytes() == want.times.tobytes() and got.ids.tobytes() == want.ids.tobytes()
    c = got.shape_cols
    if c.desc_dim:
        assert got.feats[:, c.stride - c.desc_dim:].tobytes() == want.feats[:, c.stride - c.desc_dim:].tobytes()
    assert np.all(got.shape_status == 0)
    for i, p in enumerate(pts):
        b = so.bounds(p, _abi.ROMAN_SEG_BLOCK_MIN)
        assert np.all(np.abs(got.feats[i, :3] - want.feats[i, :3]) <= b["center"])
        if c.pca >= 0:
            assert np.all(np.abs(got.feats[i, c.pca:c.pca + 3] - want.feats[i, c.pca:c.pca + 3]) <= b["ratio"])
        if c.volume >= 0:
            assert abs(got.feats[i, c.volume] - want.feats[i, c.volume]) <= b["volume"]
        if c.extent >= 0:
            assert np.all(np.abs(got.feats[i, c.extent:c.extent + 3] - want.feats[i, c.extent:c.extent + 3]) <= b["extent"])


def test_bottom_middle_ransac_table_and_pool_are_exact(ctx, world):
    clouds, pts, trajectory, times = world
    reg = RansacReg()
    reg.set_context(ctx)
    got = MapTable.from_point_clouds(reg, clouds, center_ref="bottom_middle", ctx=ctx)
    want = MapTable.from_segments(reg, oracle_segments(clouds, pts, "bottom_middle"))
    assert got.feats.shape == (60, 3) and got.feats.tobytes() == want.feats.tobytes()
    params = SubmapParams(max_size=12, radius=15.0, distance=10.0)
    centers = submap_centers(trajectory, times, params)
    a = build_submap_pool(reg, got, centers, params, ctx=ctx)
    b = build_submap_pool(reg, want, centers, params, ctx=ctx)
    assert a.pool.cpu().numpy().tobytes() == b.pool.cpu().numpy().tobytes()
    assert a.count.tobytes() == b.count.tobytes() and a.src.tobytes() == b.src.tobytes() and a.ids.tobytes() == b.ids.tobytes()
    assert a.count.sum() > 0


def test_caller_given_columns_and_minimal_segments(ctx, world, tmp_path):
    clouds, pts, trajectory, times = world
    reg = registrations()["sevg"]
    reg.set_context(ctx)
    rng = np.random.default_rng(1)
    vol, ext = rng.uniform(1.0, 2.0, 60), rng.uniform(0.1, 3.0, (60, 3))
    base = MapTable.from_point_clouds(reg, clouds, ctx=ctx)
    got = MapTable.from_point_clouds(reg, clouds, ctx=ctx, volume=vol, extent=ext)
    c = got.shape_cols
    assert np.array_equal(got.feats[:, c.volume], vol) and np.array_equal(got.feats[:, c.extent:c.extent + 3], np.sort(ext, axis=1))
    mask = np.ones(c.stride, dtype=bool); mask[c.volume] = False; mask[c.extent:c.extent + 3] = False
    assert got.feats[:, mask].tobytes() == base.feats[:, mask].tobytes()
    # the host-side callers over a table that came from clouds
    segs = clouds.minimal_segments(base)
    params = SubmapParams(max_size=12, radius=15.0, distance=10.0)
    pool = build_submap_pool(reg, base, submap_centers(trajectory, times, params), params, ctx=ctx)
    submaps = pool.to_submaps(segs)
    assert len(submaps) == len(pool.nonempty) and all(len(s.segments) for s in submaps)
    from roman_amd.align.submap_align import write_submaps_json
    write_submaps_json(str(tmp_path / "robot.sm.json"), "robot", segs, submaps)


# ---------------------------------------------------------------------------------------------
# the tolerance leg: method='roman', mean centres, through submap_align_pools
# ---------------------------------------------------------------------------------------------
def decision_margin(orc, P, D1, D2):
    """The smallest distance of any scoring decision of the problem (D1, D2) from its threshold, computed here on the ORACLE side
    with the formulas of oracle/clipper_oracle.c (pair_score with the gravity-guided form, the fusion of pair and single
    scores): l1, l2 against mindist; c against epsilon; the fused score against affinityeps.  The ratio gates compare with
    ratio_epsilon = 0 and cannot be close for positive features (asserted); the cosine gate reads descriptors only, which are the
    host's in both tables."""
    assert all(P.ratio_epsilon[f] == 0.0 for f in range(P.ratio_feature_dim)) and P.gravity_guided and P.gravity_mode == _abi.ROMAN_GRAV_COMBINED
    n1, n2 = len(D1), len(D2)
    assert np.all(D1[:, 3:3 + P.ratio_feature_dim] > 1e-9) and np.all(D2[:, 3:3 + P.ratio_feature_dim] > 1e-9)
    A = np.stack(np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij"), axis=-1).reshape(-1, 2)
    so_ = orc.single_scores(P, D1, D2)
    a, b = D1[A[:, 0], :3], D2[A[:, 1], :3]
    da, db = a[:, None, :] - a[None, :, :], b[:, None, :] - b[None, :, :]
    ok = (A[:, None, 0] != A[None, :, 0]) & (A[:, None, 1] != A[None, :, 1])         # the distinctness rule: other combinations are never scored
    h1, h2 = np.hypot(da[..., 0], da[..., 1]), np.hypot(db[..., 0], db[..., 1])
    l1, l2 = np.sqrt(h1 * h1 + da[..., 2] ** 2), np.sqrt(h2 * h2 + db[..., 2] ** 2)
    cv = np.maximum(np.abs(da[..., 2] - db[..., 2]) - np.sin(P.gravity_unc_ang_rad) * np.maximum(h1, h2), 0.0)
    c = np.sqrt((h1 - h2) ** 2 + cv * cv)
    m = min(np.abs(l1 - P.mindist)[ok].min(), np.abs(l2 - P.mindist)[ok].min(), np.abs(c - P.epsilon)[ok].min())
    live = ok & (l1 >= P.mindist) & (l2 >= P.mindist) & (c < P.epsilon) & (so_[:, None] > 0) & (so_[None, :] > 0)
    if live.any():
        fused = np.cbrt(np.exp(-0.5 * c * c / (P.sigma * P.sigma)) * so_[:, None] * so_[None, :])
        m = min(m, np.abs(fused - P.affinityeps)[live].min())
    return float(m)


def test_mean_mode_roman_alignment_is_unchanged(ctx, world, orc):
    """submap_align_pools (method='roman': pca + volume + semantics, gravity) over pools from the DEVICE table and from the ORACLE
    table of the same map, aligned against a second mapping of the same place (its own clouds, hence centres and shapes that differ
    by sampling noise): the same pairs registered, the same association arrays for every registered pair, the same loop-closure
    pairs.  The condition that makes this a fair demand is checked on the oracle side, for seed 8300 / 8301 / 8302: no submap
    membership or prune order (tests/_submaps_oracle.borderline) and no scoring decision of any pair of non-empty submaps, registered or not (decision_margin),
    lies within 1e-9 of its threshold.  The gate of pass 1 reads the trajectory only, which the two runs share.  A seed that
    fails the condition is an error of the test's input (choose another), never a reason to relax the comparison."""
    import _submaps_oracle as smo
    from roman_amd.align import submap_align as sa
    clouds, pts, trajectory, times = world
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=12)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    centers = submap_centers(trajectory, times, params)
    # the second mapping: the same segments, other samples of their surfaces
    rng = np.random.default_rng(8302)
    pts2 = [q + rng.normal(0.0, 0.02, q.shape) for q in pts]
    clouds2 = SegmentClouds(np.vstack(pts2), clouds.seg_off, clouds.ids, clouds.times, clouds.descriptors)
    dev_t = MapTable.from_point_clouds(reg, clouds, ctx=ctx)
    ora_t = MapTable.from_segments(reg, oracle_segments(clouds, pts))
    other_t = MapTable.from_segments(reg, oracle_segments(clouds2, pts2))
    assert dev_t.feats.tobytes() != ora_t.feats.tobytes(), "the two tables are identical: the leg would show nothing"
    prune_by_time = params.pruning_method == 'time'
    for t in (ora_t, other_t):
        flags = smo.borderline(t.feats, t.times, centers.descs(), max_size=params.max_size, prune_by_time=prune_by_time, radius=params.radius, tol=1e-9)
        assert not flags, f"borderline submap membership, choose another seed: {flags[:3]}"
    pool = {k: build_submap_pool(reg, t, centers, params, ctx=ctx) for k, t in (("dev", dev_t), ("ora", ora_t), ("other", other_t))}
    assert np.array_equal(pool["dev"].count, pool["ora"].count) and np.array_equal(pool["dev"].src, pool["ora"].src)
    got = sa.submap_align_pools(p, [pool["dev"], pool["other"]], io, registration=reg)
    want = sa.submap_align_pools(p, [pool["ora"], pool["other"]], io, registration=reg)
    # the oracle side: every pair's decisions keep 1e-9 from their thresholds
    P = reg._abi_params()
    rows = {k: pool[k].pool.cpu().numpy() for k in ("ora", "other")}
    sub = lambda k, s: rows[k][s * pool[k].cap: s * pool[k].cap + pool[k].count[s]]
    n = want.clipper_num_associations
    k0, k1 = pool["ora"].nonempty, pool["other"].nonempty
    assert n.shape == (len(k0), len(k1))
    worst = np.inf
    for i, s0 in enumerate(k0):
        for j, s1 in enumerate(k1):
            if pool["ora"].count[s0] >= 2 and pool["other"].count[s1] >= 2:
                worst = min(worst, decision_margin(orc, P, sub("ora", s0), sub("other", s1)))
    assert worst > 1e-9, f"a scoring decision lies {worst} from its threshold on the oracle side: choose another seed"
    # the comparison, exact
    assert np.array_equal(got.clipper_num_associations, n, equal_nan=True)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    assert np.array_equal(np.isnan(got.T_ij_hat_mat), np.isnan(want.T_ij_hat_mat))          # the same pairs registered and estimated
    for i in range(n.shape[0]):
        for j in range(n.shape[1]):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    assert np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
    assert (n >= 4).sum() >= 3 and len(want.lc_edges["pairs"]) >= 3, "hardly a pair aligned: the comparison would show nothing"
    print(f"{n.shape} grid, {(n > 0).sum()} pairs with associations, {len(want.lc_edges['pairs'])} loop closures, smallest decision margin {worst:.3g}")
