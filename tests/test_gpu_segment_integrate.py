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
identical bytes; slots are filled with a sentinel beforehand and nothing past out_count[j] changes.

What the planted cases cover beyond random clouds (the clouds are tests/_integrate_clouds.py's):
  the merge class at its real cut   jobs of 4097, 8192, 8193 and 4100 + 8200 points at the DEFAULT cuts, where the chunk is
                                    ROMAN_INTEGRATE_LDS_MAX = 4096 pairs: chunks that fill the team's LDS, a last chunk of one pair,
                                    a run without a sibling in a merge pass, the voxel sums over the global ping-pong, and a
                                    threshold and compaction over m > 4096 points — each held to the oracle, to the chunks of 64
                                    and to a second call.
  the staging edges of the search   m = 1023, 1024, 1025 (1024 columns are staged at a time, 256 queries are one workgroup's).
  keys planted on voxel faces       `faces` puts every quotient (p - origin) / vs within a rounding of an integer, at three voxel
                                    sizes, as a new segment, as a posed observation and at 5000 points through the merge class.
                                    tests/test_integrate_oracle_cpu.py shows on the CPU that a multiplication by 1 / vs changes voxel
                                    indices of every one of these clouds (and none of a random blob): a kernel that divides
                                    cheaply fails here bit for bit.
  both sides of the RANGE edge      a span of 2^21 - 1 voxels — the last that fits, key 2^63 - 1 on all three axes — is OK, 2^21
                                    is RANGE; as two points through one wave and, padded, through the two workgroup classes."""
from types import SimpleNamespace

import numpy as np
import pytest

import _integrate_oracle as io
from _integrate_clouds import FACE_CORNER, FACE_SIZES, SPAN_AXES, VS, blob, body, faces, lattice, pose, span_padded, span_pair
from roman_amd import _abi
from roman_amd.align import SegmentClouds
from roman_amd.map import IntegrationParams, cleanup_points, integrate
from roman_amd.runtime import integrate_jobs, integrate_params, integrate_slots

pytestmark = pytest.mark.gpu

GUARD = -7.25e300
CUTS = {"wave": (4096, 4096), "default": (0, 0), "merge": (16, 64)}      # every job in one wave | the default classes | chunks of 64 merged
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, 256, 257)
STAGES = (1023, 1024, 1025)               # around the 1024 columns k_integ_knn_tile stages at a time: one stage | exactly one | a second of one column
LDS_MAX = _abi.ROMAN_INTEGRATE_LDS_MAX


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


def case_stages():
    """m = n at the staging edges of the workgroup search"""
    clouds = [lattice(n, n, (-1.0, 2.0, 0.3)) for n in STAGES]
    return SimpleNamespace(name="stages", clouds=clouds, jobs=[(None, k, None) for k in range(len(clouds))], poses=None)


def case_merge(n):
    """One new segment beyond the default LDS cut: a lattice (m = n) at 4097, blobs of 30 voxels a side at 8192 and 8193."""
    cloud = lattice(n, n, (-1.0, 2.0, 0.3)) if n == 4097 else blob(n, n, 30.0, FACE_CORNER)
    return SimpleNamespace(name=f"merge{n}", clouds=[cloud], jobs=[(None, 0, None)], poses=None, merged=[0])


def case_merge_two():
    """A base of 4100 points with a posed observation of 8200 (pose 1 of two), and new segments of 300 and of 200 points: the
    merging workgroup, the LDS workgroup and one wave in one call."""
    T = pose(12300)
    whole = blob(12300, 12300, 34.0, FACE_CORNER)
    clouds = [whole[:4100], body(whole[4100:], T), blob(12301, 300, 7.0, (-2.0, 0.0, 1.0)), blob(12302, 200, 6.0, (0.0, 4.0, 0.0))]
    return SimpleNamespace(name="merge_two", clouds=clouds, jobs=[(0, 1, 1), (None, 2, None), (None, 3, None)], poses=np.array([pose(12299), T]), merged=[0])


def case_faces(vs):
    """600 points on voxel faces as a new segment and as a posed observation onto an empty base (the assembled coordinates are
    then a rounding away from the faces); at the file's voxel size also 5000 points in 24 voxels a side: the merge class at the
    default cuts, many points per voxel."""
    T = pose(600)
    p = faces(600, 600, FACE_CORNER, 12, vs)
    clouds, jobs = [p, np.zeros((0, 3)), body(p, T)], [(None, 0, None), (1, 2, 0)]
    if vs == VS:
        clouds, jobs = clouds + [faces(5000, 5000, FACE_CORNER, 24, vs)], jobs + [(None, 3, None)]
    return SimpleNamespace(name=f"faces{vs}", clouds=clouds, jobs=jobs, poses=np.array([T]), vs=vs)


def case_span(padded):
    """Per SPAN_AXES a cloud whose span is the last that fits (index KEY_TOP: jobs 0-3) and one beyond it (jobs 4-7); as two
    points, or padded with 300 points next to the first corner."""
    clouds = [span_padded(40 + k, t, axes) if padded else span_pair(t, axes) for t in (io.KEY_TOP, io.KEY_TOP + 1) for k, axes in enumerate(SPAN_AXES)]
    return SimpleNamespace(name="span_padded" if padded else "span", clouds=clouds, jobs=[(None, k, None) for k in range(len(clouds))], poses=None)


MERGE = ("merge4097", "merge8192", "merge8193", "merge_two")
FACES = tuple(f"faces{vs}" for vs in FACE_SIZES)
CASES = {c.name: c for c in (case_sizes(), case_large(600), case_large(2500), case_mixed(), case_stages(), case_merge(4097), case_merge(8192),
                             case_merge(8193), case_merge_two(), *(case_faces(vs) for vs in FACE_SIZES), case_span(False), case_span(True))}
_ORACLE = {}


def sizes_of(case):
    """n(base) + n(add) per job: what the host cuts the classes by"""
    return [(0 if b is None else len(case.clouds[b])) + len(case.clouds[a]) for b, a, _ in case.jobs]


def oracle(name, std):
    """The oracle's answer per job of a case, computed once."""
    if (name, std) not in _ORACLE:
        c = CASES[name]
        P = io.params(getattr(c, "vs", VS), std)
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
        return ctx.segment_integrate(integrate_params(getattr(case, "vs", VS), std), pts, off, case.jobs, case.poses, out_points=np.full((total, 3), GUARD),
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
    """A cloud of n points as a new segment and as base + posed observation, through one wave, the LDS workgroup (both sizes lie
    below the default cut of 4096 points, so the default is the LDS class for both) and the merging workgroup with chunks of 64.
    The merge at the default cuts, from 4097 points on, is test_merge_class_at_the_default_cuts'."""
    case = CASES[f"large{n}"]
    off = run(ctx, case, None)
    check_off(case, off)
    on = run(ctx, case, 1.0)
    check_on(case, on, 1.0)
    assert same(on, run(ctx, case, 1.0))
    for cuts in ("wave", "merge"):
        assert same(off, run(ctx, case, None, cuts)) and same(on, run(ctx, case, 1.0, cuts)), f"the {cuts} class differs"


def through_every_class(ctx, case):
    """Held to the oracle at the default cuts, step off and on; then a second call and both other cut settings give the same bytes."""
    off = run(ctx, case, None)
    check_off(case, off)
    on = run(ctx, case, 1.0)
    check_on(case, on, 1.0)
    assert same(on, run(ctx, case, 1.0)) and same(off, run(ctx, case, 0.0)), "two calls differ"
    for cuts in ("wave", "merge"):
        assert same(off, run(ctx, case, None, cuts)) and same(on, run(ctx, case, 1.0, cuts)), f"the {cuts} class differs"
    return off, on


@pytest.mark.parametrize("name", MERGE)
def test_merge_class_at_the_default_cuts(ctx, name):
    """The merging workgroup as the mapper reaches it: chunks of ROMAN_INTEGRATE_LDS_MAX pairs.  4097 = one full chunk and one of
    a single pair, m = n; 8192 = two full chunks, one pass; 8193 = three runs and two passes, the third run without a sibling in
    the first; 4100 + 8200 posed points with an LDS-class and a wave-class job in the same call.  Every merged job is past the
    cut by n and by m (the threshold and the compaction then run over m > 4096 too)."""
    case = CASES[name]
    n, ms = sizes_of(case), [len(r.down) for r in oracle(name, 1.0)]
    assert all(n[j] > LDS_MAX and ms[j] > LDS_MAX for j in case.merged), (n, ms)
    if name == "merge_two":
        assert n == [3 * LDS_MAX + 12, 300, 200] and _abi.ROMAN_INTEGRATE_WAVE_MAX < n[1] <= LDS_MAX and n[2] <= _abi.ROMAN_INTEGRATE_WAVE_MAX
    else:
        assert n[0] == {"merge4097": LDS_MAX + 1, "merge8192": 2 * LDS_MAX, "merge8193": 2 * LDS_MAX + 1}[name] and (name != "merge4097" or ms[0] == n[0])
    through_every_class(ctx, case)


def test_staging_edges_of_the_neighbour_search(ctx):
    """m = 1023, 1024, 1025 down-sampled points: no second stage of columns, none either with the first one full, and a second
    stage of one column with a fifth query tile of one valid query — through the workgroup search (default) and the wave's."""
    case = CASES["stages"]
    assert [len(r.down) for r in oracle("stages", 1.0)] == list(STAGES) == sizes_of(case) and STAGES[1] == 1024 and max(STAGES) <= LDS_MAX
    through_every_class(ctx, case)


@pytest.mark.parametrize("name", FACES)
def test_keys_planted_on_voxel_faces(ctx, name):
    """Every quotient (p - origin) / vs of these clouds lies within a rounding of an integer, so the voxel a point falls in
    depends on the correctly rounded subtraction and division (tests/test_integrate_oracle_cpu.py: the reciprocal moves points
    of every one of them).  Bit for bit with the oracle, in every class."""
    case = CASES[name]
    if case.vs == VS:
        assert sizes_of(case)[2] > LDS_MAX
    off, _ = through_every_class(ctx, case)
    assert off.count[0] < 600 and off.count[1] < 600              # points share voxels: the sums are not trivial


def test_the_last_span_that_fits(ctx):
    """Voxel index 2^21 - 1 on an axis is the last the key holds — on all three axes the key is 2^63 - 1, one below the padding
    key's top bit — and 2^21 is RANGE: two points through one wave, then padded to 302 points through the LDS workgroup (default)
    and the merging one."""
    top = np.full(3, VS * (io.KEY_TOP - 0.5))
    idx = io.voxel_indices(CASES["span_padded"].clouds[0], VS)
    assert int(io.pack(idx)[1]) == 2 ** 63 - 1 and np.sum(np.all(idx == io.KEY_TOP, axis=1)) == 1
    for name in ("span", "span_padded"):
        case = CASES[name]
        assert [r.status for r in oracle(name, None)] == [io.OK] * 4 + [io.RANGE] * 4
        assert all(_abi.ROMAN_INTEGRATE_WAVE_MAX < n <= LDS_MAX for n in sizes_of(case)) if name == "span_padded" else sizes_of(case) == [2] * 8
        off, on = through_every_class(ctx, case)
        assert off.status.tolist() == on.status.tolist() == [io.OK] * 4 + [io.RANGE] * 4
        assert np.all(off.count[4:] == 0) and np.all(on.count[4:] == 0) and np.all(off.points[off.slot[4]:] == GUARD) and np.all(on.points[on.slot[4]:] == GUARD)
        for j, axes in enumerate(SPAN_AXES):
            far = case.clouds[j][1]
            got = off.cloud(j)
            assert np.sum(np.all(got == far, axis=1)) == 1, (name, j, "the far point is alone in its voxel and comes back as it is")
            if name == "span":
                assert off.count[j] == 2 and got.tobytes() == case.clouds[j].tobytes() and on.count[j] == 0
            else:
                assert on.count[j] == off.count[j] - 1 and not np.any(np.all(on.cloud(j) == far, axis=1)), (name, j, "the far point alone is an outlier")
        assert off.cloud(0)[-1].tobytes() == top.tobytes() and off.cloud(1)[-1].tobytes() == CASES[name].clouds[1][1].tobytes()      # sorted last: x is the most significant


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
