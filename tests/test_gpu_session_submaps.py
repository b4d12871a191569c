"""roman_session_submaps_dev / roman_session_submaps on the device against roman_submaps_dev called per map on the
same device, through the C ABI.

Everything is compared BITWISE per robot: the slice [sub_off[r], sub_off[r+1]) of count, status and desc_out and the slice
[sub_off[r]*cap, sub_off[r+1]*cap) of pool, src and ids_out equal, byte for byte, what the per-map call leaves in outputs filled
with the same sentinels — so the rows beyond count[g] and the descriptor of an empty submap are held to "not written" too —, and the
guard regions around every output are intact.  No tolerance anywhere: both sides run the same per-submap code on the same numbers."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import _session_submaps as sx
import _submaps_oracle as so
from _hipmem import Hip
from roman_amd import _abi
from test_gpu_submaps import FILL, Guarded, oracle, run_dev, sparams

pytestmark = pytest.mark.gpu


def make_map(seed, N, F, S, ensure=True, **kw):
    """A seeded map table with ids; with `ensure`, segment 0 sits at the first centre at its time: submap 0 is not empty."""
    feats, times, descs = so.random_map(np.random.default_rng(seed), N, F, S, **kw)
    if ensure and N and S:
        feats[0, :3] = descs[0]["pos"] + 0.25
        times[0] = descs[0]["time"]
        for k in range(1, min(kw.get("coincide", 0), N - 1) + 1):               # (the copies of segment 0 stay copies)
            feats[k, :3] = feats[0, :3]; times[k] = times[0]
    return feats, times, np.arange(N, dtype=np.int64) * 3 + 5 + 100000 * seed, descs


def run_session(ctx, hip, P, maps, d=0, shift=0, with_ids=True, host=False):
    """The session call over guarded outputs -> dict of raw host arrays (`shift`: 8-byte words the pool and the table are moved off
    their 16-byte alignment).  host: the host-pointer form over arrays filled with the same sentinels."""
    t = sx.session_of([(m[0], m[1], m[2] if with_ids else None, m[3]) for m in maps])
    F = maps[0][0].shape[1]
    N, S = int(t["seg_off"][-1]), int(t["sub_off"][-1])
    rows, Fo = S * P.cap, P.point_dim + F - 3
    if host:
        r = ctx.session_submaps(P, t["seg_off"], t["feats"], t["times"], t["sub_off"], t["descs"], seg_ids=t["ids"], desc_dim=d,
                                pool=np.full((rows, Fo), FILL["pool"]), src=np.full(rows, FILL["src"], np.int32),
                                ids_out=np.full(rows, FILL["ids"], np.int64) if with_ids else None, desc_out=np.full((S, d), FILL["desc"]) if d else None)
        return dict(pool=r.pool, count=r.count, src=r.src, status=r.status, ids=r.ids, desc=r.desc), t
    dF = hip.upload(np.concatenate([np.zeros(shift), t["feats"].ravel()])) + 8 * shift
    dT = hip.upload(t["times"]); dI = hip.upload(t["ids"]) if with_ids else None
    out = dict(pool=Guarded(hip, rows * Fo, np.float64, FILL["pool"], shift), count=Guarded(hip, S, np.int32, FILL["count"]),
               src=Guarded(hip, rows, np.int32, FILL["src"]), status=Guarded(hip, S, np.int32, FILL["status"]),
               ids=Guarded(hip, rows, np.int64, FILL["ids"]) if with_ids else None, desc=Guarded(hip, S * d, np.float64, FILL["desc"]) if d else None)
    ctx.session_submaps_dev(P, F, t["seg_off"], dF if N else None, dT if N else None, t["sub_off"], t["descs"], out["pool"].ptr, out["count"].ptr,
                            out["src"].ptr, out["status"].ptr, seg_ids_ptr=dI, ids_out_ptr=out["ids"].ptr if with_ids else None, desc_dim=d,
                            desc_out_ptr=out["desc"].ptr if d else None)
    ctx.sync()
    got = {k: (v.get() if v is not None else None) for k, v in out.items()}      # (get() holds the guard regions to their sentinel)
    got["pool"] = got["pool"].reshape(rows, Fo)
    if d:
        got["desc"] = got["desc"].reshape(S, d)
    return got, t


def per_map(ctx, hip, P, maps, d=0, shift=0, with_ids=True):
    return [run_dev(ctx, hip, P, m[0], m[1], m[3], m[2] if with_ids else None, d, shift=shift) for m in maps]


def same_bytes(P, got, t, refs, tag=""):
    """Every robot's slices of the session's outputs are the per-map call's outputs, byte for byte."""
    cap = P.cap
    for r, ref in enumerate(refs):
        lo, hi = int(t["sub_off"][r]), int(t["sub_off"][r + 1])
        for name, a, b in (("count", got["count"][lo:hi], ref["count"]), ("status", got["status"][lo:hi], ref["status"]),
                           ("src", got["src"][lo * cap:hi * cap], ref["src"].reshape(-1)), ("pool", got["pool"][lo * cap:hi * cap], ref["pool"])):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, r, name)
        if ref["ids"] is not None:
            assert got["ids"][lo * cap:hi * cap].tobytes() == ref["ids"].tobytes(), (tag, r, "ids")
        if ref["desc"] is not None:
            assert got["desc"][lo:hi].tobytes() == ref["desc"].tobytes(), (tag, r, "desc")
        n = int(t["seg_off"][r + 1] - t["seg_off"][r])
        if n and hi > lo:
            assert ref["count"].max() > 0, (tag, r, "the map has no non-empty submap: nothing was compared")
            assert ref["src"][ref["src"] != FILL["src"]].max() < n


# (N_r, S_r) per robot: R in {1, 2, 3}; a map without segments and a map without centres in the middle of the list; unequal N_r, so that a
# wrong segment offset reads another map's rows; 63 rows in front, so that with an odd F map 1 starts at 8 mod 16
GRID = [[(257, 3)], [(63, 1), (65, 3)], [(1, 3), (64, 1)], [(64, 3), (0, 1), (257, 1)], [(65, 1), (257, 0), (63, 3)], [(257, 3), (0, 0), (1, 1)],
        [(63, 3), (257, 3), (65, 1)], [(0, 3), (65, 3)]]


@pytest.mark.parametrize("v", [0, 1, 2], ids=["F3", "F23-odd", "F24-shifted"])
def test_grid_of_sessions_equals_the_per_map_call(ctx, v):
    """Every list of GRID with one of the three row widths (centres only; 3 + 4 + 16, odd: a map behind an odd number of rows starts
    at 8 mod 16; an even width whose rows meet the 16-byte path unaligned once the buffers are shifted by one word), both prunings,
    with and without a radius and a time window."""
    hip = Hip()
    try:
        F, pd, d = [(3, 3, 0), (23, 3, 16), (24, 2, 16)][v]
        P = sparams(pd, max_size=[40, 7, None][v], cap=[None, None, 12][v], by_time=(v == 1), radius=[15.0, None, 20.0][v])
        for k, shape in enumerate(GRID):
            maps = [make_map(100 * k + 10 * r + v + 1, N, F, S, time_threshold=[np.inf, 60.0, np.inf][v]) for r, (N, S) in enumerate(shape)]
            if v == 1 and len(shape) > 1 and shape[0][0] % 2:
                assert (shape[0][0] * F * 8) % 16 == 8
            got, t = run_session(ctx, hip, P, maps, d, shift=int(v == 2))
            same_bytes(P, got, t, per_map(ctx, hip, P, maps, d, shift=int(v == 2)), f"{shape} F={F}")
    finally:
        hip.free_all()


def test_candidate_counts_around_max_size_and_exact_ties(ctx):
    hip = Hip()
    try:
        maps = [make_map(7, 257, 23, 3, coincide=6), make_map(8, 120, 23, 2, coincide=4), make_map(9, 65, 23, 3)]
        P0 = sparams(3, max_size=None, cap=257, radius=15.0)
        members = [oracle(P0, m[0], m[1], m[3], None, 0) for m in maps]
        assert all(0 in o["src"][0] and 1 in o["src"][0] and 2 in o["src"][0] for o in members[:2]), "the tied segments are not candidates"
        counts = sorted({int(c) for o in members for c in o["count"] if c > 2})
        assert len(counts) >= 3
        ties = 0
        for by_time in (False, True):
            for max_size in (counts[0] - 1, counts[0], counts[len(counts) // 2], counts[-1], counts[-1] + 5):
                P = sparams(3, max_size=max_size, by_time=by_time, radius=15.0)
                got, t = run_session(ctx, hip, P, maps, 16)
                refs = per_map(ctx, hip, P, maps, 16)
                same_bytes(P, got, t, refs, f"max_size={max_size} time={by_time}")
                kept = refs[0]["src"][0][:int(refs[0]["count"][0])]
                at = np.nonzero(kept == 0)[0]
                if len(at) and at[0] + 7 <= len(kept):           # key ties: the copies of segment 0 in map order, next to each other
                    assert kept[at[0]:at[0] + 7].tolist() == list(range(7)), kept
                    ties += 1
        assert ties >= 4, "no case kept the tied segments"
    finally:
        hip.free_all()


def test_candidates_beyond_lds_take_their_own_scratch_slices(ctx):
    """Two maps of 5 000 candidates per submap (no radius, an infinite time window: above the 4096 of LDS), a small map between
    them: five scratch slices at 0, 904, 1808, 1808 (the small map's: empty) and 2712.  Ordered (ranks over LDS and scratch) and in
    map order with truncation (max_size <= 0: the list as it stands, cut at cap beyond LDS)."""
    hip = Hip()
    try:
        maps = [make_map(21, 5000, 3, 2), make_map(22, 65, 3, 1), make_map(23, 5000, 3, 2)]
        whole = sparams(3, max_size=None, cap=5000)
        for m in (maps[0], maps[2]):
            assert (oracle(whole, m[0], m[1], m[3], None, 0)["count"] == 5000).all() and 5000 > 4096
        for P in (sparams(3, max_size=40), sparams(3, max_size=40, by_time=True), sparams(3, max_size=None, cap=4500), sparams(3, max_size=0, cap=50)):
            got, t = run_session(ctx, hip, P, maps)
            refs = per_map(ctx, hip, P, maps)
            same_bytes(P, got, t, refs, f"max_size={P.max_size} cap={P.cap}")
            if P.max_size <= 0:
                assert (refs[0]["status"] == so.ST_TRUNCATED).all() and (refs[1]["status"] == (so.ST_TRUNCATED if P.cap < 65 else so.ST_OK)).all()
                assert refs[0]["src"][0, :P.cap].tolist() == list(range(P.cap))
    finally:
        hip.free_all()


def test_two_runs_and_the_host_form_give_the_same_bytes(ctx):
    hip = Hip()
    try:
        maps = [make_map(31, 257, 23, 3), make_map(32, 0, 23, 1), make_map(33, 65, 23, 2)]
        P = sparams(3, max_size=20, radius=15.0)
        a, t = run_session(ctx, hip, P, maps, 16, shift=1)
        b, _ = run_session(ctx, hip, P, maps, 16, shift=1)
        h, _ = run_session(ctx, hip, P, maps, 16, host=True)
        assert a["count"].max() > 0
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
            assert a[k].reshape(-1).tobytes() == np.ascontiguousarray(h[k]).reshape(-1).tobytes(), ("host form", k)
        same_bytes(P, a, t, per_map(ctx, hip, P, maps, 16))
        no_pool = ctx.session_submaps(P, t["seg_off"], t["feats"], t["times"], t["sub_off"], t["descs"], want_pool=False)
        assert no_pool.pool is None and no_pool.ids is None and np.array_equal(no_pool.count, a["count"])
        assert np.array_equal(no_pool.src[no_pool.src >= 0], a["src"][a["src"] != FILL["src"]])
    finally:
        hip.free_all()


def test_error_codes_and_empty_calls_on_a_context(ctx):
    import test_session_submaps_abi as abi
    lib = ctx._lib
    abi.check_error_codes(lib, ctx._h)
    for host in (False, True):
        assert abi.Args(n=(), s=()).call(lib, host, ctx._h) == _abi.ROMAN_OK          # R == 0
        assert abi.Args(n=(5, 7), s=(0, 0)).call(lib, host, ctx._h) == _abi.ROMAN_OK  # no submap anywhere: nothing is dereferenced


def test_a_scratch_that_cannot_be_had_is_nomem_and_the_context_lives(ctx):
    """64 submaps over a map of 2^31 - 1 rows: 1.1 TB of candidate keys.  The call answers ROMAN_E_NOMEM in front of any launch (the
    pointers are never read), and the next call on the context works."""
    import test_session_submaps_abi as abi
    hip = Hip()
    try:
        big = abi.Args(n=((1 << 31) - 1,), s=(64,), alloc=False)
        some = hip.alloc(4096)
        rc = ctx._lib.roman_session_submaps_dev(ctx._h, C.byref(big.P), 1, 6, big.seg_off.ctypes.data, some, some, None, big.sub_off.ctypes.data,
                                                np.zeros(64, dtype=big.a["descs"].dtype).ctypes.data, some, some, some, None, some, 0, None)
        assert rc == _abi.ROMAN_E_NOMEM, (rc, ctx._lib.roman_last_error(ctx._h))
        maps = [make_map(41, 65, 3, 2), make_map(42, 64, 3, 1)]
        P = sparams(3, max_size=10)
        got, t = run_session(ctx, hip, P, maps)
        same_bytes(P, got, t, per_map(ctx, hip, P, maps))
    finally:
        hip.free_all()


# ---------------------------------------------------------------------------------------------
# end to end: torch holds the device memory, so this runs in a process of its own with torch imported first
# ---------------------------------------------------------------------------------------------
D = 16


def run_end_to_end():
    import torch
    import _session as ss
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_session_pools, build_submap_pool, submap_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40,
                          submap_descriptor='mean_semantic', submap_descriptor_thresh=0.65, single_robot_lc_time_thresh=60.0)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    base = synth.make_map(300, D, seed=41, n_poses=60, dt=4.0)
    views = [dict(keep=1.0, first_pose=0, last_pose=None), dict(keep=0.85, first_pose=8, last_pose=None), dict(keep=0.9, first_pose=0, last_pose=50)]
    tables, centers = [], []
    for r, v in enumerate(views):
        segs, traj, times = ss.robot_view(*base, r, d=D, **v)
        tables.append(MapTable.from_segments(reg, segs)); centers.append(submap_centers(traj, times, params))
    pools = build_session_pools(reg, tables, centers, params, ctx=ctx, device=dev)
    apart = [build_submap_pool(reg, t, c, params, ctx=ctx, device=dev) for t, c in zip(tables, centers)]
    assert len({len(t) for t in tables}) == 3 and len({len(c) for c in centers}) >= 2
    for got, want in zip(pools, apart):
        sx.same_pool(got, want)
        assert len(got.nonempty) >= 4
    sx.one_storage(pools, "pool"); sx.one_storage(pools, "ids_dev"); sx.one_storage(pools, "desc_dev")
    assert sa._one_storage(torch, [q.pool for q in pools]).data_ptr() == pools[0].pool.data_ptr() and sa._one_storage(torch, [q.pool for q in apart]) is None
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=40.0)
    got = sa.submap_align_session(p, pools, None, io, registration=reg)
    want = sa.submap_align_session(p, apart, None, io, registration=reg)
    assert list(got) == list(want) == [(r, s) for r in range(3) for s in range(r, 3)]
    aligned = edges = 0
    for key in want:
        ss.compare(got[key], want[key])
        n = want[key].clipper_num_associations
        aligned += int((n >= 4).sum()); edges += len(want[key].lc_edges["pairs"])
        if key[0] == key[1]:
            assert np.all(np.diag(got[key].clipper_num_associations) == 0), "a submap against itself keeps segments: the shared-segment removal did not run"
    assert aligned >= 6 and edges >= 3, "hardly a pair aligned: the comparison would show nothing"
    ctx.close()
    print(f"{aligned} pairs aligned, {edges} loop closures\nSESSION_SUBMAPS_OK")


def test_session_pools_to_loop_closures_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_session_submaps as t; t.run_end_to_end()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_SUBMAPS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
