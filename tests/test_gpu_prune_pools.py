"""method='clipper+prune' over device-resident pools on the device: submap_align_pools / submap_align_session with
the device-prefilter plugin (DistRegWithPruning.on_device()) on a hand-made world of four places, 22 m apart, that two robots map
(submaps of at most 12 objects, 16-d descriptors).  torch holds the device memory, so the comparison runs in a process of its own
with torch imported first (as tests/test_gpu_submap_align_pools.py does).

Robot 0 drives the four places and then places 0 and 1 again (a second lap: new segment ids, 1000 s later — its pool against itself
closes loops between the laps, and neighbouring submaps of a lap share segments, so rows pass through the gather region).  Robot 1
drives the four places once; its copy of the world carries the plants:
  place 1   half of the objects have a fifth of the volume: a shape ratio alone (0.2 < epsilon_shape 0.3) removes their associations;
  place 2   every object is rolled 8 degrees about the centre: the estimate's roll is above roll_pitch_thresh (5 degrees);
  place 3   the descriptors lie in a subspace orthogonal to robot 0's there: the prefilter removes EVERY association of the pair,
            and the all-to-all list is scored instead (the rule of clipperpy for an empty list).

First expectation, for the device-prefilter plugin: submap_align_pools equals submap_align_grid over to_submaps() of the same pools —
counts, nearby matrix, association arrays and accepted pairs exactly, poses and edges within 1e-12, angles and distances within
1e-9 (tests/_session.compare: the bounds tests/test_gpu_submap_align_pools.py holds between the two paths) — and every block of
submap_align_session equals submap_align_pools.  Second expectation, for the factory's host-prefilter plugin (the reference's NumPy
product) through submap_align_grid over the same submaps: the same association sets and accepted edges, poses within 1e-12.  The two
prefilters add the 16 products of a descriptor pair in different orders, so they may disagree only where a product lies on the
threshold: `margins()` asserts on the CPU, before anything is compared, that no raw product of any two objects of the world lies
within 1e-9 of cos_min and no shape ratio within 1e-9 of epsilon_shape."""
import copy
import subprocess
import sys

import numpy as np
import pytest

D = 16
COS_MIN, EPS_SHAPE = 0.75, 0.3
N_PLACES, PER_PLACE, SPACING = 4, 9, 22.0
LAP = 1000.0
TILT_PLACE, SHAPE_PLACE, ORTHO_PLACE = 2, 1, 3
ROLL_DEG = 8.0
CASES = ["cross-radius", "cross-aabb", "self-shared-ids", "session"]


def make_world():
    """-> (objects of every place: list of dicts, place centres (4, 3)).  Descriptors: one of 6 unit prototypes in the first 8
    dimensions (two of them share a component: products near 0, 0.5 and 1) plus a little noise; shape attributes 1 or 2 (ratios
    0.5 and 1) with a per-cent of noise."""
    rng = np.random.default_rng(7)
    e = np.eye(D)
    protos = [(e[a] + e[b]) / np.sqrt(2.0) for a, b in ((0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 0))]
    centres = np.array([[SPACING * k, 0.0, 0.0] for k in range(N_PLACES)])
    places = []
    for k in range(N_PLACES):
        pts = []
        while len(pts) < PER_PLACE:
            c = centres[k] + np.array([rng.uniform(-9.0, 9.0), rng.uniform(-9.0, 9.0), rng.uniform(-1.0, 2.0)])
            if all(np.linalg.norm(c - q) >= 2.0 for q in pts):
                pts.append(c)
        objs = []
        for c in pts:
            v = protos[int(rng.integers(0, len(protos)))] + 0.05 * rng.standard_normal(D) / np.sqrt(D)
            objs.append(dict(center=c, shape=rng.choice([1.0, 2.0], size=4) * (1.0 + 0.01 * rng.standard_normal(4)), desc=v / np.linalg.norm(v)))
        places.append(objs)
    return places, centres


def _segment(sid, o, t, rng, plant=None, centre=None, k_in_place=0):
    """One robot's sighting of object `o` at time `t`: the centre a few cm off, the descriptor slightly off, plants applied."""
    from roman_amd import synth
    c = o["center"] + rng.normal(0.0, 0.03, 3)
    shape = o["shape"] * (1.0 + 0.01 * rng.standard_normal(4))
    v = o["desc"] + 0.02 * rng.standard_normal(D) / np.sqrt(D)
    if plant == "tilt":
        a = np.deg2rad(ROLL_DEG)
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
        c = centre + Rx @ (c - centre)
    if plant == "shape" and k_in_place % 2 == 0:
        shape = shape * np.array([0.2, 1.0, 1.0, 1.0])
    if plant == "ortho":
        v = np.roll(v, 8)                                    # the first 8 dimensions into the last 8
    sg = synth.SyntheticSegment(sid, c, shape[0], shape[1], shape[2], shape[3], np.ones(3), v / np.linalg.norm(v))
    sg.first_seen, sg.last_seen = float(t - 2.0), float(t + 2.0)
    return sg


def robot_map(r):
    """-> (segments, trajectory, times) of robot r over make_world()."""
    from roman_amd.synth import yaw_transform
    places, centres = make_world()
    rng = np.random.default_rng(100 + r)
    visits = [(k, 30.0 * k) for k in range(N_PLACES)] + ([(0, LAP), (1, LAP + 30.0)] if r == 0 else [])
    plants = {TILT_PLACE: "tilt", SHAPE_PLACE: "shape", ORTHO_PLACE: "ortho"} if r == 1 else {}
    segs, traj, times = [], [], []
    for v, (k, t) in enumerate(visits):
        for q, o in enumerate(places[k]):
            segs.append(_segment(100000 * r + 1000 * v + q, o, t, rng, plants.get(k), centres[k], q))
        traj.append(yaw_transform(0.4 * v + 1.1 * r, centres[k] + rng.normal(0.0, 0.2, 3) * (1.0, 1.0, 0.1), roll=0.02 * np.sin(v + r), pitch=0.02 * np.cos(v)))
        times.append(t)
    return segs, traj, np.array(times)


def margins(maps, reg):
    """No raw descriptor product of any two objects of the maps within 1e-9 of cos_min, no shape ratio within 1e-9 of
    shape_epsilon -> (smallest distance of a product, of a ratio)."""
    allsegs = [s for m in maps for s in m[0]]
    V = np.array([np.asarray(s.semantic_descriptor, dtype=np.float64) for s in allsegs])
    S = np.array([reg._object_shape_attributes(s) for s in allsegs])
    prod = V @ V.T
    ratio = np.minimum(S[:, None, :], S[None, :, :]) / np.maximum(S[:, None, :], S[None, :, :])
    dp, dr = float(np.min(np.abs(prod - reg.cos_min))), float(np.min(np.abs(ratio - reg.shape_epsilon)))
    assert dp > 1e-9, f"a raw descriptor product lies within {dp} of cos_min: the two prefilters may disagree there"
    assert dr > 1e-9, f"a shape ratio lies within {dr} of shape_epsilon"
    return dp, dr


def same_sets_and_edges(dev, host):
    """The second expectation: the device prefilter against the reference's NumPy prefilter on the same submaps."""
    n = host.clipper_num_associations
    assert np.array_equal(dev.clipper_num_associations, n, equal_nan=True)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]
    for i in range(n.shape[0]):
        for j in range(n.shape[1]):
            a, b = np.asarray(dev.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(host.associated_objs_mat[i][j]).reshape(-1, 2)
            assert np.array_equal(order(a), order(b)), (i, j)
    np.testing.assert_allclose(dev.T_ij_hat_mat, host.T_ij_hat_mat, rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(dev.lc_edges["pairs"], host.lc_edges["pairs"])
    np.testing.assert_allclose(dev.lc_edges["t"], host.lc_edges["t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dev.lc_edges["q"], host.lc_edges["q"], rtol=0, atol=1e-12)


def place_of(pool):
    """The place every non-empty submap of the pool is centred on."""
    x = pool.centers.pose_flu[pool.nonempty][:, 0, 3]
    return np.rint(x / SPACING).astype(int)


def build(ctx, device, build_ctx=None):
    """-> (params, io, device plugin, host plugin, pools, maps)."""
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p = SubmapAlignParams(method="clipper+prune", semantics_dim=D, cosine_min=COS_MIN, epsilon_shape=EPS_SHAPE, submap_radius=15.0,
                          submap_center_dist=10.0, submap_center_time=50.0, submap_max_size=12, single_robot_lc_time_thresh=200.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=50.0)
    host = p.get_object_registration(); host.set_context(ctx)             # the factory's plugin: NumPy prefilter, as the reference
    reg = host.on_device(D)
    params = SubmapParams.from_submap_align_params(p)
    maps = [robot_map(0), robot_map(1)]
    print("margins (product, ratio):", margins(maps, reg))
    pools = [build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=build_ctx or ctx, device=device)
             for sg, traj, times in maps]
    assert [len(q.nonempty) for q in pools] == [6, 4] and all(q.cap == 12 and int(q.pool.shape[1]) == 3 + 4 + D for q in pools)
    return p, io, reg, host, pools, maps


def run_case(name, built, compute=None, set_rows=lambda n: None):
    """`compute`: a CPU double for submap_align_grid (stand-in runs); `set_rows(n)`: tells a stand-in context how many rows the pools hold."""
    from roman_amd.align import submap_align as sa
    import _session as ss
    p, io, reg, host, pools, maps = built
    p = copy.copy(p)
    if name == "session":
        blocks = [(0, 0), (0, 1)]
        set_rows(sum(int(q.pool.shape[0]) for q in pools))
        got = sa.submap_align_session(p, pools, blocks, io, registration=reg)
        assert list(got) == blocks
        for r, s in blocks:
            q = copy.copy(p); q.single_robot_lc = (r == s)
            set_rows(int(pools[r].pool.shape[0]) + (0 if r == s else int(pools[s].pool.shape[0])))
            want = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
            ss.compare(got[(r, s)], want)
            assert (want.clipper_num_associations >= 4).sum() >= 2 and len(want.lc_edges["pairs"]) >= 1, (r, s)
        assert np.all(np.diag(got[(0, 0)].clipper_num_associations) == 0), "a submap against itself keeps segments"
        print("session: blocks", {k: int((v.clipper_num_associations >= 4).sum()) for k, v in got.items()})
        return
    self_case = name == "self-shared-ids"
    if name == "cross-aabb":
        p.submap_radius = None                               # the bounding-box gate, over radius-mode pools
    p.single_robot_lc = self_case
    pl = [pools[0], pools[0]] if self_case else pools
    sg = [maps[0][0], maps[0][0]] if self_case else [m[0] for m in maps]
    set_rows(int(pools[0].pool.shape[0]) if self_case else sum(int(q.pool.shape[0]) for q in pools))
    got = sa.submap_align_pools(p, pl, io, registration=reg)
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pl, sg)], io, registration=reg, compute=compute)
    ref = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pl, sg)], io, registration=host, compute=compute)
    # ---- the conditions, on the reference's side, so that nothing below compares nothing ----
    n = ref.clipper_num_associations
    assert (n >= 4).sum() >= 2, "fewer than two pairs aligned with 4 associations"
    assert len(ref.lc_edges["pairs"]) >= 1 and np.isnan(n).sum() == 0 and (np.isnan(ref.robots_nearby_mat)).any()
    subs = [q.to_submaps(s) for q, s in zip(pl, sg)]
    if self_case:
        shared = sum(len({s.id for s in a.segments} & {s.id for s in b.segments}) > 0 for i, a in enumerate(subs[0]) for j, b in enumerate(subs[1]) if i != j)
        assert shared >= 4 and np.all(np.diag(n) == 0), "no two submaps share segments, or a submap against itself keeps some"
        lap = (pools[0].centers.time[pools[0].nonempty] >= LAP).astype(int)
        acc = np.asarray(ref.lc_edges["pairs"]).reshape(-1, 2)
        assert len(acc) >= 2 and np.all(lap[acc[:, 0]] != lap[acc[:, 1]]), "fewer than two loops close between the laps, or one inside a lap"
    else:
        k0, k1 = place_of(pools[0]), place_of(pools[1])
        at = lambda place: (int(np.nonzero(k0 == place)[0][0]), int(np.nonzero(k1 == place)[0][0]))
        # the all-pruned pair: the reference's prefilter keeps NOTHING, the all-to-all list is scored, and the pair aligns
        i, j = at(ORTHO_PLACE)
        assert len(host._associations_to_score(subs[0][i].segments, subs[1][j].segments)) == 0, "the prefilter left a survivor in the all-pruned pair"
        assert n[i, j] >= 4
        # the shape pair: associations whose product passes and whose volume ratio alone does not
        i, j = at(SHAPE_PLACE)
        a, b = subs[0][i].segments, subs[1][j].segments
        prod = np.array([x.semantic_descriptor for x in a]) @ np.array([x.semantic_descriptor for x in b]).T
        loose = copy.copy(host); loose.shape_epsilon = 0.0
        assert len(host._associations_to_score(a, b)) < len(loose._associations_to_score(a, b)) <= int((prod >= COS_MIN).sum()), "no association fell to a shape ratio alone"
        assert n[i, j] >= 4
        # the tilt pair: rejected by the plugin's roll / pitch check, and aligned without it
        i, j = at(TILT_PLACE)
        assert n[i, j] == 0 and np.isnan(ref.T_ij_hat_mat[i, j]).all(), "the tilt plant was not rejected"
        lenient = copy.copy(reg); lenient.roll_pitch_thresh = np.deg2rad(20.0)
        free = sa.submap_align_pools(p, pl, io, registration=lenient)
        assert free.clipper_num_associations[i, j] >= 4, "the tilt plant does not align even without the roll / pitch check"
        if name == "cross-aabb":
            c0, c1 = (q.centers.pose_flu[q.nonempty][:, :3, 3] for q in pools)
            radius_near = np.linalg.norm(c0[:, None] - c1[None], axis=2) < 30.0
            assert (~np.isnan(ref.robots_nearby_mat) != radius_near).any(), "NEARBY under boxes equals the radius gate: a gate without boxes would pass"
    ss.compare(got, want)                                    # first expectation: pools == grid, the device plugin on both
    same_sets_and_edges(got, ref)                            # second: the device prefilter == the reference's NumPy prefilter
    print(f"{name}: grid {n.shape}, {len(got.timing_list)} pairs registered, {int((n >= 4).sum())} aligned, {len(ref.lc_edges['pairs'])} loop closures")


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    built = build(ctx, dev)
    for name in CASES:
        run_case(name, built)
    ctx.close()
    print("PRUNE_POOLS_OK")


@pytest.mark.gpu
def test_clipper_prune_over_pools_and_session_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_prune_pools as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "PRUNE_POOLS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
