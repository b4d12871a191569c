"""The four forms of submap extraction — single map, force-fill (§4.12), session (§4.19), session list (§4.21) — share
ONE job table: one pinned staging and one device table per context, written by every call.  What can go wrong there is a stale or a
short table left by the previous call, so the forms are interleaved on one context and every result is held, byte for byte, to the
same call on a context that has seen nothing else; the single-map edges that now run through the session's code are held to the
NumPy restatement (tests/_submaps_oracle.py), the fill form behind a larger radius call to tests/_fill_boxes_oracle.py.

Every call is a host-pointer call over NumPy arrays of the shapes the C ABI names: nothing here hands the library a pointer it may not
read or write."""
import numpy as np
import pytest

import _fill_boxes_oracle as fo
import _session_submaps as sx
import _submaps_oracle as so
from roman_amd import _abi
from roman_amd.runtime import Context
from test_gpu_session_submaps import make_map
from test_gpu_submaps import FILL, check, clean_map, oracle, sparams

pytestmark = pytest.mark.gpu

F, CAP, D = 6, 4, 2


def outputs(S, cap, Fo, d, ids=True):
    """Output arrays filled with the sentinels: what a call leaves untouched is compared too."""
    rows = S * cap
    return dict(pool=np.full((rows, Fo), FILL["pool"]), src=np.full(rows, FILL["src"], np.int32),
                ids_out=np.full(rows, FILL["ids"], np.int64) if ids else None, desc_out=np.full((S, d), FILL["desc"]) if d else None)


def fields(r):
    return dict(pool=r.pool, count=r.count, src=r.src, ids=r.ids, status=r.status, desc=r.desc)


def same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k)


def single(c, P, m, d=D):
    """The single-map call over the map m = (feats, times, ids, descs) -> the dict test_gpu_submaps.check() reads."""
    feats, times, ids, descs = m
    S = len(descs)
    g = fields(c.submaps(P, feats, times, descs, seg_ids=ids, desc_dim=d, **outputs(S, P.cap, P.point_dim + feats.shape[1] - 3, d)))
    g["src"] = g["src"].reshape(S, P.cap); g["ids"] = g["ids"].reshape(S, P.cap)
    return g


def test_interleaved_forms_on_one_context_equal_fresh_contexts(ctx):
    P = sparams(3, max_size=CAP, radius=15.0)
    maps = [make_map(61 + r, N, F, S) for r, (N, S) in enumerate([(5, 2), (0, 3), (7, 1)])]     # map 1: submaps but no segments
    t = sx.session_of(maps)
    one = make_map(71, 7, F, 2)
    filled = make_map(72, 7, F, 5)
    rng = np.random.default_rng(73)
    fcount = np.array([4, 0, 3, 1, 4], np.int32); fsrc = rng.integers(0, 7, (5, CAP)).astype(np.int32)
    changed_maps = list(maps)
    m2 = maps[2]
    changed_maps[2] = (m2[0] + np.where(np.arange(F) >= 3, 0.5, 0.0), m2[1], m2[2] + 1, m2[3])   # other columns and ids, the same centres
    t2 = sx.session_of(changed_maps)
    lst = np.array([0, 4], np.int32)

    def session(c):
        return fields(c.session_submaps(P, t["seg_off"], t["feats"], t["times"], t["sub_off"], t["descs"], seg_ids=t["ids"], desc_dim=D,
                                        **outputs(6, CAP, F, D)))

    def fill(c):
        r = c.submaps_fill(3, CAP, filled[0], filled[3], fcount, fsrc, seg_ids=filled[2], desc_dim=D)
        return dict(pool=r.pool, ids=r.ids, desc=r.desc)

    def listed(c, base):
        cur = {k: v.copy() for k, v in base.items()}
        r, chg = c.session_submaps_list(P, t2["seg_off"], t2["feats"], t2["times"], t2["sub_off"], t2["descs"], lst, cur["pool"], cur["count"], cur["src"],
                                        cur["status"], seg_ids=t2["ids"], ids_out=cur["ids"], desc_dim=D, desc_out=cur["desc"])
        return dict(fields(r), changed=chg)

    steps = [("session", session), ("single", lambda c: single(c, P, one)), ("fill", fill), ("list", None), ("single again", lambda c: single(c, P, one))]
    got = {}
    for name, call in steps:                                     # all five on the shared context, in this order
        got[name] = call(ctx) if call else listed(ctx, got["session"])
    assert got["session"]["count"].max() > 0 and got["single"]["count"].max() > 0 and (got["session"]["count"][2:5] == 0).all()
    for name, call in steps:                                     # each on a context of its own
        fresh = Context(0)
        try:
            want = call(fresh) if call else listed(fresh, got["session"])
        finally:
            fresh.close()
        same(got[name], want, name)
    # the unlisted slots kept the first session's bytes — slot 5, map 2's, although its inputs changed —; a listed slot is written whole
    for g in (1, 2, 3, 5):
        for k, per in (("pool", CAP), ("count", 1), ("src", CAP), ("ids", CAP), ("status", 1), ("desc", 1)):
            assert got["list"][k][g * per:(g + 1) * per].tobytes() == got["session"][k][g * per:(g + 1) * per].tobytes(), (g, k)
    n0 = int(got["session"]["count"][0])
    assert got["list"]["count"][0] == n0 and (got["list"]["src"][n0:CAP] == -1).all() and (got["list"]["pool"][n0:CAP] == 0.0).all()
    same(got["single again"], got["single"], "the same call twice")


def test_single_map_edges_through_the_session_path(ctx):
    ids = lambda N: np.arange(N, dtype=np.int64) * 3 + 5
    # no segments: count 0, status OK, nothing of the pool written (check() holds the rows beyond count to the sentinel)
    P = sparams(3, max_size=CAP, radius=15.0)
    feats, times, descs = so.random_map(np.random.default_rng(81), 0, F, 2)
    g = single(ctx, P, (feats, times, ids(0), descs))
    check(P, oracle(P, feats, times, descs, ids(0), D), g, "N=0")
    assert g["count"].tolist() == [0, 0] and g["status"].tolist() == [_abi.ROMAN_ST_OK] * 2 and (g["pool"] == FILL["pool"]).all()
    # no submaps
    feats, times, descs = so.random_map(np.random.default_rng(82), 7, F, 0)
    g = single(ctx, P, (feats, times, ids(7), descs))
    check(P, oracle(P, feats, times, descs, ids(7), D), g, "S=0")
    assert g["count"].shape == (0,) and g["pool"].shape == (0, F) and g["desc"].shape == (0, D)
    # one candidate more than the on-chip list holds, everything kept: submap s spills one entry, into entry s of the scratch
    N = _abi.SUBMAP_LDS_CAND + 1
    assert N == 4097
    P = sparams(3, max_size=None, cap=8, radius=1e6)
    feats, times, descs = clean_map(83, N, F, 3, P)
    o = oracle(P, feats, times, descs, ids(N), D)
    assert (o["status"] == _abi.ROMAN_ST_ASSOC_TRUNCATED).all() and all(o["src"][s].tolist() == list(range(8)) for s in range(3))
    check(P, o, single(ctx, P, (feats, times, ids(N), descs)), "N=4097 map order")
    # ... and ranked over the on-chip list and the spill together: the spilled candidate is the nearest of submap 2
    P = sparams(3, max_size=8, radius=1e6)
    feats[N - 1, :3] = descs[2]["pos"]
    assert not so.borderline(feats, times, descs, max_size=8, radius=1e6)
    o = oracle(P, feats, times, descs, ids(N), D)
    assert o["src"][2, 0] == N - 1 and (o["count"] == 8).all() and (o["status"] == _abi.ROMAN_ST_OK).all()
    check(P, o, single(ctx, P, (feats, times, ids(N), descs)), "N=4097 ranked")


def test_fill_behind_a_radius_call_of_more_submaps(ctx):
    """The radius call leaves five records in the job table, the fill call needs two: its rows are the host's lists all the same."""
    P = sparams(3, max_size=CAP, radius=15.0)
    big = make_map(91, 7, F, 5)
    assert single(ctx, P, big)["count"].max() > 0
    feats, _, ids, descs = make_map(92, 7, F, 2)
    slices = [[6, 0, 3], [2, 2, 5, 1]]
    want = fo.fill_oracle(feats, descs, slices, CAP, point_dim=3, seg_ids=ids, desc_dim=D)
    r = ctx.submaps_fill(3, CAP, feats, descs, want["count"], want["src"], seg_ids=ids, desc_dim=D)
    for s, sl in enumerate(slices):
        n = len(sl)
        assert r.pool[s * CAP:s * CAP + n].tobytes() == want["rows"][s].tobytes(), s
        assert np.all(r.pool[s * CAP + n:(s + 1) * CAP] == 0.0) and np.all(r.ids[s * CAP + n:(s + 1) * CAP] == -1)
        assert np.array_equal(r.ids[s * CAP:s * CAP + n], want["ids"][s])
    assert r.desc.tobytes() == want["desc"].tobytes()
