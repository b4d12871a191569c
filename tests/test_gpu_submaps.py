"""roman_submaps_dev / roman_submaps on the device against the NumPy restatement of the contract (tests/_submaps_oracle.py) and
the reference's own output (tests/golden/submaps_golden.npz), through the C ABI.

Compared exactly: count, src, ids_out, status and every column but the centre (bit for bit).  The centre: 1e-12 * max(1, |c|) —
a few ulps of three products and three sums at coordinates up to 1e3 (1 ulp of 1e3 is 1.1e-13), not a measured number.
Descriptors: 1e-12.  Generated maps carry no borderline flag (the generator moves on to the next seed otherwise)."""
import numpy as np
import pytest

import _submaps_oracle as so
from _hipmem import Hip
from roman_amd import _abi

pytestmark = pytest.mark.gpu

G = 64                                       # guard elements on either side of every output
FILL = dict(pool=-7.25, src=-77, ids=-777, desc=-5.5, count=-3, status=-3)


def sparams(point_dim=3, max_size=None, cap=None, by_time=False, radius=None):
    P = _abi.RomanSubmapParams()
    P.point_dim = point_dim; P.max_size = max_size or 0; P.cap = max_size if max_size else cap
    P.prune_by_time = int(by_time); P.use_radius = int(radius is not None); P.radius = radius if radius is not None else 0.0
    return P


def clean_map(seed, N, F, S, P, **kw):
    """A seeded map without borderline flags for the parameters P."""
    for k in range(20):
        feats, times, descs = so.random_map(np.random.default_rng(seed + 1000 * k), N, F, S, **kw)
        if not so.borderline(feats, times, descs, max_size=P.max_size or None, prune_by_time=bool(P.prune_by_time),
                             radius=P.radius if P.use_radius else None):
            return feats, times, descs
    raise AssertionError("no clean map in 20 seeds")


def oracle(P, feats, times, descs, ids, d):
    return so.submaps_oracle(feats, times, descs, point_dim=P.point_dim, max_size=P.max_size or None, cap=P.cap, prune_by_time=bool(P.prune_by_time),
                             radius=P.radius if P.use_radius else None, seg_ids=ids, desc_dim=d)


class Guarded:
    """A device array between two guard regions, everything filled with a sentinel."""

    def __init__(self, hip, n, dtype, fill, shift=0):
        self.hip, self.n, self.dtype, self.fill, self.lead = hip, int(n), np.dtype(dtype), fill, G + shift
        self.base = hip.upload(np.full(self.n + 2 * G + shift, fill, dtype=dtype))
        self.ptr = self.base + self.lead * self.dtype.itemsize

    def get(self):
        whole = self.hip.download(self.base, (self.n + self.lead + G,), self.dtype)
        assert (whole[:self.lead] == self.fill).all() and (whole[self.lead + self.n:] == self.fill).all(), "a guard region was written"
        return whole[self.lead:self.lead + self.n].copy()


def run_dev(ctx, hip, P, feats, times, descs, ids=None, d=0, shift=0):
    """roman_submaps_dev over guarded outputs -> dict of host arrays (`shift`: 8-byte words the pool and the table are moved off
    their 16-byte alignment)."""
    N, F = feats.shape
    S, rows, Fo, shift = len(descs), len(descs) * P.cap, P.point_dim + F - 3, int(shift)
    dF = hip.upload(np.concatenate([np.zeros(shift), feats.ravel()])) + 8 * shift
    dT = hip.upload(times); dI = hip.upload(ids) if ids is not None else None
    out = dict(pool=Guarded(hip, rows * Fo, np.float64, FILL["pool"], shift), count=Guarded(hip, S, np.int32, FILL["count"]),
               src=Guarded(hip, rows, np.int32, FILL["src"]), status=Guarded(hip, S, np.int32, FILL["status"]),
               ids=Guarded(hip, rows, np.int64, FILL["ids"]) if ids is not None else None,
               desc=Guarded(hip, S * d, np.float64, FILL["desc"]) if d else None)
    ctx.submaps_dev(P, N, F, dF if N else None, dT if N else None, descs, out["pool"].ptr, out["count"].ptr, out["src"].ptr, out["status"].ptr,
                    seg_ids_ptr=dI, ids_out_ptr=out["ids"].ptr if ids is not None else None, desc_dim=d, desc_out_ptr=out["desc"].ptr if d else None)
    ctx.sync()
    got = {k: (v.get() if v is not None else None) for k, v in out.items()}
    got["pool"] = got["pool"].reshape(rows, Fo); got["src"] = got["src"].reshape(S, P.cap)
    if got["ids"] is not None:
        got["ids"] = got["ids"].reshape(S, P.cap)
    if got["desc"] is not None:
        got["desc"] = got["desc"].reshape(S, d)
    return got


def check(P, o, got, tag=""):
    S = len(o["count"])
    assert np.array_equal(got["count"], o["count"]), (tag, got["count"], o["count"])
    assert np.array_equal(got["status"], o["status"]), tag
    pd = P.point_dim
    for s in range(S):
        n = int(o["count"][s])
        assert np.array_equal(got["src"][s, :n], o["src"][s, :n]), (tag, s)
        assert (got["src"][s, n:] == FILL["src"]).all(), (tag, s, "src beyond count written")
        rows = got["pool"][s * P.cap:(s + 1) * P.cap]
        want = o["rows"][s]
        err = np.abs(rows[:n, :pd] - want[:, :pd])
        print(f"{tag} submap {s}: n={n} max centre error {err.max() if n else 0.0:.3e}")
        assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(want[:, :pd]))), (tag, s)
        assert rows[:n, pd:].tobytes() == want[:, pd:].tobytes(), (tag, s, "a copied column differs")
        assert (rows[n:] == FILL["pool"]).all(), (tag, s, "pool rows beyond count written")
        if o["ids"] is not None:
            assert np.array_equal(got["ids"][s, :n], o["ids"][s]) and (got["ids"][s, n:] == FILL["ids"]).all(), (tag, s)
        if got["desc"] is not None:
            if n:
                assert np.all(np.abs(got["desc"][s] - o["desc"][s]) <= 1e-12), (tag, s)
            else:
                assert (got["desc"][s] == FILL["desc"]).all(), (tag, s, "descriptor of an empty submap written")


SHAPES = [(N, S) for N in (0, 1, 63, 64, 65, 257, 1000) for S in (0, 1, 3)]


@pytest.mark.parametrize("N,S", SHAPES)
def test_shapes_against_the_oracle(ctx, N, S):
    """Every N x S of the list, each with the three row widths (centres only; 3 + 4 + 16; an even width whose rows meet the
    16-byte path unaligned once the buffers are shifted by one word), both prunings, with and without a radius."""
    hip = Hip()
    try:
        for v, (F, pd, d) in enumerate([(3, 3, 0), (23, 3, 16), (24, 2, 16)]):
            P = sparams(pd, max_size=[40, 7, None][v], cap=[None, None, 12][v], by_time=(v == 1), radius=[15.0, None, 20.0][v])
            feats, times, descs = clean_map(100 * N + 10 * S + v, N, F, S, P, time_threshold=[np.inf, 60.0, np.inf][v])
            ids = np.arange(N, dtype=np.int64) * 3 + 5
            got = run_dev(ctx, hip, P, feats, times, descs, ids, d, shift=(v == 2))
            check(P, oracle(P, feats, times, descs, ids, d), got, f"N={N} S={S} F={F}")
    finally:
        hip.free_all()


def test_candidate_counts_around_max_size_empty_submap_and_truncation(ctx):
    hip = Hip()
    try:
        P0 = sparams(3, max_size=None, cap=257, radius=15.0)
        feats, times, descs = clean_map(4242, 257, 23, 3, P0)
        descs[2]["pos"] += 1000.0                                               # a centre no segment is near
        members = oracle(P0, feats, times, descs, None, 0)["count"]
        assert members[0] > 8 and members[1] > 8 and members[0] != members[1] and members[2] == 0
        lo, hi = sorted(int(m) for m in members[:2])
        for by_time in (False, True):
            for max_size in (lo - 3, lo, hi + 5):                               # above, equal to and below the candidate counts
                P = sparams(3, max_size=max_size, by_time=by_time, radius=15.0)
                assert not so.borderline(feats, times, descs, max_size=max_size, prune_by_time=by_time, radius=15.0)
                o = oracle(P, feats, times, descs, None, 16)
                check(P, o, run_dev(ctx, hip, P, feats, times, descs, None, 16), f"max_size={max_size} time={by_time}")
        assert lo - 3 < lo < hi + 5 and o["count"][2] == 0
        P = sparams(3, max_size=None, cap=lo - 1, radius=15.0)                  # no max_size, slots smaller than the membership
        o = oracle(P, feats, times, descs, None, 16)
        assert (o["status"][:2] == _abi.ROMAN_ST_ASSOC_TRUNCATED).all() and o["status"][2] == 0
        check(P, o, run_dev(ctx, hip, P, feats, times, descs, None, 16), "truncated")
    finally:
        hip.free_all()


def test_more_candidates_than_the_on_chip_list_holds(ctx):
    """5000 candidates per submap against the 4096 the select kernel keeps in LDS: the others go through the context's scratch,
    for the ranking (max_size set) and for the map-order copy (max_size absent, slots of 4500 rows: truncated)."""
    hip = Hip()
    try:
        N = 5000
        assert N > _abi.SUBMAP_LDS_CAND
        for P in (sparams(3, max_size=50), sparams(3, max_size=4500, by_time=True), sparams(3, max_size=None, cap=4500)):
            feats, times, descs = clean_map(77, N, 3, 2, P)
            ids = np.arange(N, dtype=np.int64)[::-1].copy()
            o = oracle(P, feats, times, descs, ids, 0)
            assert (o["count"] == min(P.cap, N)).all()
            if P.max_size:
                assert (o["src"][:, :P.cap] >= _abi.SUBMAP_LDS_CAND).any(), "no selected row comes from the spilled part of the list"
            check(P, o, run_dev(ctx, hip, P, feats, times, descs, ids, 0), f"spill max_size={P.max_size}")
    finally:
        hip.free_all()


def test_exact_ties_keep_map_order_and_calls_are_deterministic(ctx):
    hip = Hip()
    try:
        for by_time in (False, True):
            P = sparams(3, max_size=30, by_time=by_time, radius=25.0)
            feats, times, descs = clean_map(9, 200, 23, 2, P, coincide=6)       # segments 1..6 repeat segment 0's centre and times
            descs[0]["pos"] = feats[0, :3] + 0.5; T = np.eye(4); T[:3, 3] = -descs[0]["pos"]; descs[0]["T_center_odom"] = T
            descs[0]["time"] = (times[0, 0] + times[0, 1]) / 2.0
            assert not so.borderline(feats, times, descs, max_size=30, prune_by_time=by_time, radius=25.0)
            ids = np.arange(200, dtype=np.int64)[::-1].copy() * 11               # different ids, descending with the map index
            o = oracle(P, feats, times, descs, ids, 16)
            assert o["src"][0, :7].tolist() == [0, 1, 2, 3, 4, 5, 6]            # the nearest seven are the duplicates, in map order
            a = run_dev(ctx, hip, P, feats, times, descs, ids, 16)
            b = run_dev(ctx, hip, P, feats, times, descs, ids, 16)
            check(P, o, a, f"ties time={by_time}")
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), f"{k} differs between two calls"
    finally:
        hip.free_all()


def test_host_pointer_call_gives_the_same_bytes(ctx):
    hip = Hip()
    try:
        for P, d, F in ((sparams(3, max_size=12, radius=15.0), 16, 23), (sparams(2, max_size=None, cap=9, radius=18.0), 0, 8)):
            feats, times, descs = clean_map(555, 300, F, 3, P)
            descs[1]["pos"] += 500.0                                            # an empty submap: its slot and descriptor stay as they were
            ids = np.arange(300, dtype=np.int64) + 40
            dev = run_dev(ctx, hip, P, feats, times, descs, ids, d)
            S, rows, Fo = 3, 3 * P.cap, P.point_dim + F - 3
            res = ctx.submaps(P, feats, times, descs, seg_ids=ids, desc_dim=d, pool=np.full((rows, Fo), FILL["pool"]),
                              src=np.full(rows, FILL["src"], np.int32), ids_out=np.full(rows, FILL["ids"], np.int64),
                              desc_out=np.full((S, d), FILL["desc"]) if d else None)
            assert dev["count"][1] == 0 and dev["count"][0] > 0
            assert res.pool.tobytes() == dev["pool"].tobytes() and res.src.tobytes() == dev["src"].tobytes()
            assert res.ids.tobytes() == dev["ids"].tobytes() and np.array_equal(res.count, dev["count"]) and np.array_equal(res.status, dev["status"])
            if d:
                assert res.desc.tobytes() == dev["desc"].tobytes()
            check(P, oracle(P, feats, times, descs, ids, d), dev, "host parity")
            nopool = ctx.submaps(P, feats, times, descs, seg_ids=ids, desc_dim=d, want_pool=False)
            assert nopool.pool is None and np.array_equal(nopool.count, dev["count"])
            assert np.array_equal(nopool.src.reshape(S, -1)[0, :dev["count"][0]], dev["src"][0, :dev["count"][0]])
    finally:
        hip.free_all()


CASES = so.golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_on_the_device(ctx, case):
    """The reference's own submaps: membership and order exact, centres to the bound, other columns equal, descriptors to 1e-12."""
    from roman_amd.align.submaps import SubmapParams, submap_centers
    kw = case["kw"]
    centers = submap_centers(list(case["trajectory"]), case["traj_times"], SubmapParams(**kw))
    P = sparams(3, max_size=kw["max_size"], cap=len(case["feats"]), by_time=kw["pruning_method"] == 'time', radius=kw["radius"])
    res = ctx.submaps(P, case["feats"], case["times"], centers.descs(), seg_ids=case["ids"], desc_dim=16)
    assert np.array_equal(np.nonzero(res.count > 0)[0], case["sm_id"]) and not res.status.any()
    pool = res.pool.reshape(len(centers), P.cap, -1)
    for q, s in enumerate(case["sm_id"]):
        n = res.count[s]
        assert np.array_equal(res.src.reshape(len(centers), -1)[s, :n], case["src"][q]), (case["name"], s)
        want = case["cen"][q]
        assert np.all(np.abs(pool[s, :n, :3] - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
        assert np.array_equal(pool[s, :n, 3:], case["feats"][case["src"][q], 3:])
        assert np.array_equal(res.ids.reshape(len(centers), -1)[s, :n], case["ids"][case["src"][q]])
        assert np.all(np.abs(res.desc[s] - case["sm_desc"][q]) <= 1e-12)
    for s in np.nonzero(res.count == 0)[0]:
        assert np.isnan(res.desc[s]).all()


def test_bad_arguments_are_refused(ctx):
    feats, times, descs = so.random_map(np.random.default_rng(1), 10, 5, 2)
    ok = sparams(3, max_size=4, radius=5.0)
    assert ctx.submaps(ok, feats, times, descs).count.shape == (2,)
    bad = []
    P = sparams(3, max_size=4, radius=5.0); P.cap = 5; bad.append((P, 0))      # cap != max_size
    P = sparams(3, max_size=None, cap=0); bad.append((P, 0))                   # cap < 1
    P = sparams(4, max_size=4); bad.append((P, 0))                             # point_dim
    P = sparams(3, max_size=4); P.reserved0 = 1; bad.append((P, 0))
    P = sparams(3, max_size=4); P.reserved[1] = 1; bad.append((P, 0))
    bad.append((ok, 3))                                                        # desc_dim > F - 3
    for P, d in bad:
        with pytest.raises(_abi.RomanHipError) as e:
            ctx.submaps(P, feats, times, descs, desc_dim=d)
        assert e.value.code == _abi.ROMAN_E_INVALID
    assert ctx.submaps(ok, feats, times, descs).count.shape == (2,)            # the context stays usable


def test_device_pools_feed_the_batch_calls():
    """Plumbing end to end (torch for device memory: its own process, torch imported first): two pools built on the device,
    grid_batch -> align_resident, against roman_align_batch with host pointers on the SAME pool bytes copied back — associations,
    poses and status identical (only offsets and counts are under test)."""
    import subprocess, sys, textwrap
    from conftest import ROOT
    code = textwrap.dedent("""
        import sys
        import numpy as np
        import torch
        sys.path.insert(0, %r)
        from roman_amd import synth
        from roman_amd.align import SubmapAlignParams
        from roman_amd.align.pipeline import align_resident
        from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
        from roman_amd.runtime import Context
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
        ctx = Context(0, stream=stream.cuda_stream)
        reg = SubmapAlignParams(method="semanticgrav", semantics_dim=16).get_object_registration(); reg.set_context(ctx)
        params = SubmapParams(max_size=30, radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor='mean_semantic')
        pools = []
        for seed in (31, 31):                          # the same place mapped twice: cross pairs have true matches
            segs, traj, times = synth.make_map(200, 16, seed=seed, n_poses=24, dt=8.0)
            table = MapTable.from_segments(reg, segs)
            pools.append(build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=ctx, device=dev))
        batch, pool = pools[0].grid_batch(pools[1])
        assert len(batch) >= 16 and (batch.n1 > 0).all()
        got = align_resident(reg, batch, pool, ctx=ctx)
        host = pool.cpu().numpy()
        want = ctx.align_batch(reg._abi_params(), host, batch.off1, batch.n1, batch.off2, batch.n2, kmax=batch.kmax())
        for b in range(len(batch)):
            assert np.array_equal(got.assoc[b], want.assoc[b]), b
        assert np.array_equal(got.T, want.T, equal_nan=True) and np.array_equal(got.status, want.status)
        assert sum(len(a) >= 4 for a in got.assoc) >= 4, "no pair of the grid aligned: the test would show nothing"
        sms = pools[0].to_submaps(segs)
        s0 = int(pools[0].nonempty[0])
        assert np.array_equal(reg.pack(sms[0].segments), host[s0 * pools[0].cap:s0 * pools[0].cap + pools[0].count[s0]])
        ctx.close()
        print("SUBMAPS_PLUMBING_OK")
    """ % (ROOT,))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SUBMAPS_PLUMBING_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
