"""roman_segment_integrate on the device against tests/_integrate_oracle.py.

What is exact and what is bounded.  With the outlier step off, out_count, out_status and the down-sampled points are the oracle's
bit for bit: every voxel's sum has one order (input order from 0.0).  out_avg is the oracle's bit for bit: the k smallest squared
distances are a multiset, their roots are added ascending.  out_thr is held against `threshold_truth` — the formula in
np.longdouble on the device's own out_avg — within the bound derived there from the depth of the fixed summation order
(ceil(m / 64) - 1 additions per lane, 6 butterfly levels).  The kept set: every point whose avg lies below truth - bound is kept,
every point above truth + bound (or with avg = 0) is dropped, points inside the band may go either way; `test_the_band_is_thin`
asserts on the oracle alone that at most 1 % of the points of this file's clouds lie in the band.  m <= 2 is the planted case of
an empty result and is asserted as such.

Every size class (one wave, a workgroup in LDS, a workgroup merging through global memory), both cut settings and two calls give
identical bytes; slots are filled with a sentinel beforehand and nothing past out_count[j] changes."""
from types import SimpleNamespace

import numpy as np
import pytest

import _integrate_oracle as io
from roman_amd import _abi
from roman_amd.align import SegmentClouds
from roman_amd.map import IntegrationParams, cleanup_points, integrate
from roman_amd.runtime import integrate_jobs, integrate_params, integrate_slots

pytestmark = pytest.mark.gpu

GUARD = -7.25e300
VS = 0.05
CUTS = {"wave": (4096, 4096), "default": (0, 0), "merge": (16, 64)}      # every job in one wave | the default classes | chunks of 64 merged
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, 256, 257)


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


# ----------------------------------------------------------------------------------------------------------------- the cases
def case_sizes():
    clouds = [lattice(n, n, (-1.0, 2.0, 0.3)) for n in SIZES] + [blob(100 + n, n, 2.0 + n ** (1 / 3)) for n in SIZES]
    return SimpleNamespace(name="sizes", clouds=clouds, jobs=[(None, k, None) for k in range(len(clouds))], poses=None)


def case_large(n):
    side = {600: 7.0, 2500: 11.0}[n]
    T = pose(n)
    whole = blob(n, n, side, (3.0, -1.0, 0.5))
    clouds = [whole, whole[:n // 3], body(whole[n // 3:], T)]
    return SimpleNamespace(name=f"large{n}", clouds=clouds, jobs=[(None, 0, None), (1, 2, 0)], poses=np.array([T]))


def case_mixed():
    T = pose(1)
    c = [blob(1, 300, 6.0), body(blob(2, 200, 6.0, (0.1, 0.0, 0.05)), T), blob(3, 150, 5.0, (2.0, 2.0, 2.0)), np.zeros((0, 3)),
         blob(4, 120, 5.0, (2.05, 2.0, 2.1)), np.zeros((0, 3)), blob(5, 80, 4.0), np.array([0.2, 0.2, 0.2]) + np.random.default_rng(6).uniform(0, 0.4, (50, 3)) * VS,
         lattice(7, 100), blob(8, 90, 4.0, (-2.0, 0.0, 0.0)), blob(9, 70, 4.0)]
    jobs = [(None, 9, None),        # a new segment
            (0, 1, 0),              # an associated observation: pose given
            (4, 2, None),           # a merge: no pose
            (10, 3, None),          # an empty added cloud: the base comes back unchanged
            (5, 6, None),           # an empty base
            (None, 7, None),        # all points in one voxel
            (None, 8, None)]        # every point its own voxel
    return SimpleNamespace(name="mixed", clouds=c, jobs=jobs, poses=np.array([T]))


CASES = {c.name: c for c in (case_sizes(), case_large(600), case_large(2500), case_mixed())}
_ORACLE = {}


def oracle(name, std):
    """The oracle's answer per job of a case, computed once."""
    if (name, std) not in _ORACLE:
        c = CASES[name]
        P = io.params(VS, std)
        _ORACLE[name, std] = [io.integrate(None if b is None else c.clouds[b], c.clouds[a], None if p is None else c.poses[p], P) for b, a, p in c.jobs]
    return _ORACLE[name, std]


def pack(clouds):
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.ascontiguousarray(np.vstack([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds])), off


def run(ctx, case, std, cuts="default"):
    """One call with every output filled with the sentinel beforehand."""
    pts, off = pack(case.clouds)
    n_jobs = len(case.jobs)
    total = int(integrate_slots(off, integrate_jobs(case.jobs))[-1])
    ctx.set_integrate_cuts(*CUTS[cuts])
    try:
        return ctx.segment_integrate(integrate_params(VS, std), pts, off, case.jobs, case.poses, out_points=np.full((total, 3), GUARD),
                                     out_avg=np.full(total, GUARD), out_thr=np.full(n_jobs, GUARD))
    finally:
        ctx.set_integrate_cuts(0, 0)


def same(a, b):
    return all(np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes() for f in ("points", "count", "status", "avg", "thr"))


def band(avg, std):
    """-> (truth, bound, must_keep, must_drop) of one job's mean distances"""
    truth, bound = io.threshold_truth(avg, std)
    with np.errstate(invalid="ignore"):
        return truth, bound, (avg > 0) & (avg < truth - bound), ~(avg > 0) | (avg > truth + bound) | np.isnan(truth)


def check_off(case, out):
    """outlier step off: counts, status and the down-sampled points bit for bit; the slots' tails, avg and thr untouched"""
    ref = oracle(case.name, None)
    for j, r in enumerate(ref):
        s0, s1 = out.slot[j], out.slot[j + 1]
        assert out.status[j] == r.status and out.count[j] == len(r.points), (case.name, j)
        assert out.cloud(j).tobytes() == r.points.tobytes(), (case.name, j)
        assert np.all(out.points[s0 + out.count[j]:s1] == GUARD), (case.name, j)
    assert np.all(out.avg == GUARD) and np.all(out.thr == GUARD)


def check_on(case, out, std):
    """outlier step on: avg bit for bit, thr within its bound, the kept set outside the band"""
    ref = oracle(case.name, std)
    for j, r in enumerate(ref):
        s0, s1 = out.slot[j], out.slot[j + 1]
        assert out.status[j] == r.status, (case.name, j)
        if r.avg is None:                                   # an empty added cloud (or RANGE): no clean-up ran
            assert out.count[j] == len(r.points) and out.cloud(j).tobytes() == r.points.tobytes() and out.thr[j] == GUARD, (case.name, j)
            assert np.all(out.avg[s0:s1] == GUARD) and np.all(out.points[s0 + out.count[j]:s1] == GUARD)
            continue
        m = len(r.down)
        avg = out.avg[s0:s0 + m]
        assert avg.tobytes() == r.avg.tobytes(), (case.name, j, np.abs(avg - r.avg).max())
        assert np.all(out.avg[s0 + m:s1] == GUARD) and np.all(out.points[s0 + out.count[j]:s1] == GUARD), (case.name, j)
        truth, bound, must_keep, must_drop = band(avg, std)
        print(f"{case.name} job {j}: m = {m}, thr = {out.thr[j]!r}, truth = {truth!r}, bound = {bound:.3e}, kept {out.count[j]}")
        if m <= 2:                                          # the planted consequences: avg = 0 (m = 1), std = 0 and x < x (m = 2)
            assert out.count[j] == 0 and (np.isnan(out.thr[j]) if m == 1 else out.thr[j] == avg[0]), (case.name, j)
            continue
        assert abs(out.thr[j] - truth) <= bound, (case.name, j, out.thr[j], truth, bound)
        kept, at = np.zeros(m, dtype=bool), 0               # the output is a subsequence of the down-sampled cloud, whose rows are distinct
        got = out.cloud(j)
        for i in range(m):
            if at < len(got) and got[at].tobytes() == r.down[i].tobytes():
                kept[i] = True
                at += 1
        assert at == len(got), (case.name, j, "the output is not a subsequence of the down-sampled cloud")
        assert np.all(kept[must_keep]) and not np.any(kept[must_drop]), (case.name, j)


# ----------------------------------------------------------------------------------------------------------------- the tests
def test_the_band_is_thin():
    """On the oracle alone: at most 1 % of the down-sampled points of this file's clouds lie inside the threshold's band."""
    inside = points = 0
    for name in CASES:
        for r in oracle(name, 1.0):
            if r.avg is None or len(r.avg) <= 2:
                continue
            _, _, must_keep, must_drop = band(r.avg, 1.0)
            inside += int(np.sum(~must_keep & ~must_drop))
            points += len(r.avg)
    assert points > 3000 and inside <= 0.01 * points, (inside, points)


@pytest.mark.parametrize("name", ["sizes", "mixed"])
def test_against_the_oracle(ctx, name):
    case = CASES[name]
    off = run(ctx, case, None)
    check_off(case, off)
    on = run(ctx, case, 1.0)
    check_on(case, on, 1.0)
    assert same(on, run(ctx, case, 1.0)) and same(off, run(ctx, case, 0.0)), "two calls differ"
    for cuts in ("wave", "merge"):
        assert same(off, run(ctx, case, None, cuts)) and same(on, run(ctx, case, 1.0, cuts)), f"the {cuts} class differs"


def test_sizes_are_what_they_plant():
    """m = 1, 2, 9, 10, 11 down-sampled points are among the cases, and every size sits on both sides of the default wave cut."""
    ms = [len(r.down) for r in oracle("sizes", 1.0)]
    assert ms[:len(SIZES)] == list(SIZES) and _abi.ROMAN_INTEGRATE_WAVE_MAX in SIZES and _abi.ROMAN_INTEGRATE_WAVE_MAX + 1 in SIZES
    mixed = oracle("mixed", 1.0)
    assert len(mixed[5].down) == 1 and len(mixed[6].down) == 100 and mixed[3].avg is None and len(mixed[3].points) == 70


@pytest.mark.parametrize("n", [600, 2500])
def test_large_clouds_through_every_class(ctx, n):
    """A cloud of n points as a new segment and as base + posed observation, through one wave, the LDS workgroup (2500: the merge
    at default cuts would need more than 4096 points, so the default is the LDS class for both) and the merging workgroup."""
    case = CASES[f"large{n}"]
    off = run(ctx, case, None)
    check_off(case, off)
    on = run(ctx, case, 1.0)
    check_on(case, on, 1.0)
    assert same(on, run(ctx, case, 1.0))
    for cuts in ("wave", "merge"):
        assert same(off, run(ctx, case, None, cuts)) and same(on, run(ctx, case, 1.0, cuts)), f"the {cuts} class differs"


def test_range_status_and_other_deviations(ctx):
    far = np.array([[0.0, 0.0, 0.0], [VS * 2.0 ** 21, 0.0, 0.0]])
    case = SimpleNamespace(name="range", clouds=[far, np.array([[0.0, np.nan, 0.0]]), blob(3, 40, 3.0), np.zeros((0, 3))],
                           jobs=[(None, 0, None), (None, 1, None), (None, 2, None), (None, 3, None)], poses=None)
    for std in (1.0, None, np.inf, -1.0):
        out = run(ctx, case, std)
        assert out.status.tolist() == [io.RANGE, io.RANGE, io.OK, io.EMPTY] and out.count[0] == out.count[1] == out.count[3] == 0
        assert np.all(out.points[:3] == GUARD)
    ref = io.down_sample(case.clouds[2], VS)
    assert run(ctx, case, np.inf).cloud(2).tobytes() == ref.tobytes() == run(ctx, case, None, "merge").cloud(2).tobytes()


def observation(points, T, time, desc):
    return SimpleNamespace(points=body(points, T), pose=T, time=time, semantic_descriptor=desc)


def test_three_frames_through_integrate(ctx):
    """The issue's three frames, and two more for the descriptor.  Frame 1: two new segments.  Frame 2: segment 0 is associated with an observation, a third segment is new.  Frame 3: that
    third segment is merged into segment 1 (no pose: both are in the world frame).  Frame 4: segment 0 is associated again.  Frame
    5: the merged segment (two observations behind its descriptor) is merged into segment 0.  Per segment the cloud the oracle
    returns job by job, and the descriptor `_integrate_oracle.Descriptor` keeps — the reference's lines, renormalisation included,
    over up to four successive updates."""
    P = IntegrationParams(VS, 1.0)
    oP = io.params(VS, 1.0)
    rng = np.random.default_rng(11)
    T = [pose(20 + k) for k in range(5)]
    desc = rng.normal(size=(5, 16)) * np.array([[1.0], [3.0], [0.25], [2.0], [7.0]])      # norms far from 1
    obs = [observation(blob(30, 260, 6.0), T[0], 1.0, desc[0]), observation(blob(31, 180, 5.0, (1.0, 1.0, 0.0)), T[1], 1.0, desc[1]),
           observation(blob(32, 220, 6.0, (0.05, 0.0, 0.0)), T[2], 2.0, desc[2]), observation(blob(33, 150, 5.0, (1.1, 1.0, 0.1)), T[3], 2.0, desc[3]),
           observation(blob(34, 240, 6.0, (-0.05, 0.05, 0.0)), T[4], 4.0, desc[4])]

    def added(which):
        o = [obs[k] for k in which]
        off = np.concatenate([[0], np.cumsum([len(x.points) for x in o])]).astype(np.int64)
        return SegmentClouds(np.vstack([x.points for x in o]), off, np.arange(len(o), dtype=np.int64) + 10 * which[0],
                             np.array([[x.time, x.time] for x in o]), np.stack([x.semantic_descriptor for x in o]))

    def one(c, k):
        """segment k of a SegmentClouds as a SegmentClouds of its own"""
        return SegmentClouds(c.points[c.seg_off[k]:c.seg_off[k + 1]], np.array([0, c.seg_off[k + 1] - c.seg_off[k]]), c.ids[k:k + 1], c.times[k:k + 1],
                             c.descriptors[k:k + 1])

    def exact(r, k, ref, d):
        assert r.status[k] == ref.status
        pts = r.clouds.points[r.clouds.seg_off[k]:r.clouds.seg_off[k + 1]]
        _, bound, must_keep, must_drop = band(ref.avg, 1.0)
        assert np.all(must_keep | must_drop), "a point of the scripted sequence lies in the threshold's band: choose another seed"
        assert pts.tobytes() == ref.points.tobytes() and abs(r.threshold[k] - ref.thr) <= 2 * bound
        assert r.clouds.descriptors[k].tobytes() == d.value.tobytes() and r.desc_counts[k] == d.cnt
        assert abs(np.linalg.norm(r.clouds.descriptors[k]) - 1.0) <= 4 * io.EPS

    empty = SegmentClouds(np.zeros((0, 3)), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros((0, 16)))
    # frame 1
    f1 = integrate(empty, added([0, 1]), [(None, 0, 0), (None, 1, 1)], P, poses=np.array(T[:2]), ctx=ctx)
    o0, o1 = io.integrate(None, obs[0].points, T[0], oP), io.integrate(None, obs[1].points, T[1], oP)
    d0, d1 = io.Descriptor().add(desc[0]), io.Descriptor().add(desc[1])
    exact(f1, 0, o0, d0); exact(f1, 1, o1, d1)
    assert f1.clouds.ids.tolist() == [0, 1] and f1.clouds.times.tolist() == [[1.0, 1.0], [1.0, 1.0]] and f1.desc_counts.tolist() == [1, 1]
    # frame 2: segment 0 with observation 2; observation 3 is a new segment; segment 1 is not touched
    f2 = integrate(f1.clouds, added([2, 3]), [(0, 0, 0), (None, 1, 1)], P, poses=np.array(T[2:4]), ctx=ctx, segment_counts=f1.desc_counts)
    o0, o2 = io.integrate(o0.points, obs[2].points, T[2], oP), io.integrate(None, obs[3].points, T[3], oP)
    d0.add(desc[2]); d2 = io.Descriptor().add(desc[3])
    exact(f2, 0, o0, d0); exact(f2, 1, o2, d2)
    assert f2.clouds.ids.tolist() == [0, 21] and f2.clouds.times.tolist() == [[1.0, 2.0], [2.0, 2.0]] and f2.desc_counts.tolist() == [2, 1]
    # frame 3: the new segment (f2's second) is merged into segment 1 (f1's second)
    f3 = integrate(one(f1.clouds, 1), one(f2.clouds, 1), [(0, 0)], P, ctx=ctx)
    o1 = io.integrate(o1.points, o2.points, None, oP)
    d1.add(d2.value, d2.cnt)
    exact(f3, 0, o1, d1)
    assert f3.clouds.ids.tolist() == [1] and f3.clouds.times.tolist() == [[1.0, 2.0]] and f3.desc_counts.tolist() == [2]
    # frame 4: segment 0 again, its second running mean
    f4 = integrate(one(f2.clouds, 0), added([4]), [(0, 0, 0)], P, poses=np.array(T[4:]), ctx=ctx, segment_counts=f2.desc_counts[:1])
    o0 = io.integrate(o0.points, obs[4].points, T[4], oP)
    d0.add(desc[4])
    exact(f4, 0, o0, d0)
    assert f4.clouds.times.tolist() == [[1.0, 4.0]] and f4.desc_counts.tolist() == [3]
    # frame 5: the merged segment, two observations behind its descriptor, into segment 0
    f5 = integrate(f4.clouds, f3.clouds, [(0, 0)], P, ctx=ctx, segment_counts=f4.desc_counts, added_counts=f3.desc_counts)
    o0 = io.integrate(o0.points, o1.points, None, oP)
    d0.add(d1.value, d1.cnt)
    exact(f5, 0, o0, d0)
    assert f5.clouds.ids.tolist() == [0] and f5.desc_counts.tolist() == [5]
    # cleanup_points is one job without a base
    assert cleanup_points(blob(30, 260, 6.0), P, ctx=ctx).tobytes() == io.cleanup(blob(30, 260, 6.0), oP).points.tobytes()


def test_no_job_is_ok_and_writes_nothing(ctx):
    """n_jobs = 0 returns ROMAN_OK from both forms and leaves every output as it was; the Python wrapper returns empty arrays."""
    import ctypes as C
    pts, off = pack([blob(1, 20, 3.0), blob(2, 30, 3.0)])
    P = integrate_params(VS, 1.0)
    out_points, count, status, avg, thr = np.full((50, 3), GUARD), np.full(2, -77, np.int32), np.full(2, -77, np.int32), np.full(50, GUARD), np.full(2, GUARD)
    jobs = integrate_jobs([(0, 1, None)])
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib, h = ctx._lib, ctx._h
    assert lib.roman_segment_integrate(h, C.byref(P), p(pts), p(off), 2, None, 0, p(jobs), 0, p(out_points), p(count), p(status), p(avg), p(thr)) == _abi.ROMAN_OK
    assert lib.roman_segment_integrate(h, C.byref(P), p(pts), p(off), 2, None, 0, None, 0, None, None, None, None, None) == _abi.ROMAN_OK
    # the device form returns behind the argument checks, before any device pointer is looked at
    assert lib.roman_segment_integrate_dev(h, C.byref(P), p(pts), None, p(off), 2, None, 0, None, None, 0, None, None, None, None, None) == _abi.ROMAN_OK
    ctx.sync()
    assert np.all(out_points == GUARD) and np.all(avg == GUARD) and np.all(thr == GUARD) and np.all(count == -77) and np.all(status == -77)
    r = ctx.segment_integrate(P, pts, off, [], None, want_avg=True)
    assert r.points.shape == (0, 3) and r.count.shape == (0,) and r.status.shape == (0,) and r.avg.shape == (0,) and r.thr.shape == (0,) and r.slot.tolist() == [0]
    # a call whose slots are all empty has no out_points to give
    e = ctx.segment_integrate(P, np.zeros((0, 3)), np.zeros(3, np.int64), [(None, 0), (1, 0)])
    assert e.count.tolist() == [0, 0] and e.status.tolist() == [io.EMPTY, io.EMPTY]
