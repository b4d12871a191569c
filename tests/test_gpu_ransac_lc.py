"""RANSAC loop closures on the device: roman_ransac_lc_batch[_dev] and submap_align_pools(method='ransac').

What must be bit-identical is compared as bytes: strided rows against packed rows against roman_ransac_batch_dev, the split outputs
against the record's fields, the fused tail against roman_lc_tail_dev on its own, the host-pointer form against the device form.
Against the CPU: the tail within tests/test_gpu_lc_tail.py's tolerances (tests/_lc_tail.assert_records_match); end to end,
associations and counts exact, poses, angles and distances within 1e-9 (what tests/test_gpu_submap_align_pools.py cites from
tests/test_gpu_ransac.py::test_through_the_plugin).  Every problem compared with the NumPy oracle has ZERO borderline hypotheses
under it, asserted (tests/_ransac_lc.solve, _oracle_is_clean): a borderline case fails loudly.

Shapes: n, m in 5 ... 12, max_iteration 2048, round 256, B <= 16, grids of a few submaps a side; plus n = 70 and n = 90 (3 n above
the workgroup's 256 threads: a staging loop takes a second trip)."""
import functools

import numpy as np
import pytest

import _lc_tail as lt
import _ransac_lc as rl
import _ransac_oracle as ro
import test_ransac_lc_cpu as cpu
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.align import submap_align as sa
from roman_amd.runtime import LcInputs, RomanHipError, lc_record_dtype, ransac_record_dtype

pytestmark = pytest.mark.gpu
ITER, ROUND, EDGE = 2048, 256, 0.8                  # (edge_len 0.8: a few per cent of the random triples are scored, also at n = 70 and 90)
WIDE = 3 + 4 + 16


def _params(**kw):
    k = dict(max_iteration=ITER, round=ROUND, edge_len=EDGE, max_dist=0.5, confidence=0.999, seed=0); k.update(kw)
    return _abi.RomanRansacParams(k["max_iteration"], k["round"], k["edge_len"], k["max_dist"], k["confidence"], k["seed"])


@functools.lru_cache(maxsize=None)
def _problems():
    """-> (pts (N, 3), off1, n1, off2, n2): B = 11 problems over one packed pool."""
    sets = []
    for n, m, seed in ((7, 8, 100), (8, 5, 101), (6, 6, 102), (70, 12, 103), (90, 7, 104)):
        P, Q, _, _, _ = ro.planted(n, m, seed, n_in=min(n, m, 12))
        sets += [P, Q]
    line = np.outer(np.arange(7.0), [1.0, 2.0, 0.5]) + 1.0          # collinear, and every edge of Q is 100 times an edge of P: no triple passes the edge test
    sets += [line, 100.0 * line]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int64)
    S = lambda k: (offs[k], len(sets[k]))
    prob = [(S(0), S(1)), (S(2), S(3)), (S(4), S(5)),
            (S(0), S(3)),                                           # two problems that share a slice with others
            (S(4), S(4)),                                           # off1 == off2
            ((offs[2], 0), S(1)), (S(0), (offs[5], 0)),             # an empty map on either side
            (S(10), S(11)),                                         # no survivor
            (S(6), S(7)), (S(8), S(9)),                             # 3 n > 256: the staging loop's second trip
            (S(5), S(4))]
    off1, n1 = np.array([p[0][0] for p in prob], np.int64), np.array([p[0][1] for p in prob], np.int32)
    off2, n2 = np.array([p[1][0] for p in prob], np.int64), np.array([p[1][1] for p in prob], np.int32)
    return np.vstack(sets), off1, n1, off2, n2


def _wide(pts):
    rows = np.full((len(pts), WIDE), np.nan); rows[:, :3] = pts
    return rows


@functools.lru_cache(maxsize=None)
def _oracle_is_clean():
    """Every non-empty problem of _problems() under the oracle: no borderline hypothesis.  -> {problem: the oracle's run}."""
    pts, off1, n1, off2, n2 = _problems()
    out = {}
    for b in range(len(n1)):
        if n1[b] and n2[b]:
            out[b] = ro.run(pts[off1[b]:off1[b] + n1[b]], pts[off2[b]:off2[b] + n2[b]], max_iteration=ITER, round=ROUND, edge_len=EDGE)
            assert out[b].n_border == 0, f"problem {b} has a borderline hypothesis: choose another seed"
    return out


def run_dev(ctx, rows, off1, n1, off2, n2, kmax, lc=None, counts=False, packed_call=False, rp=None, fill=0xAB):
    """One device-pointer call -> dict of host arrays (every output buffer pre-filled with `fill` bytes)."""
    rp = rp or _params(); B = len(n1); F = rows.shape[1]
    hip = Hip()
    try:
        pre = lambda nbytes: hip.upload(np.full(max(nbytes, 8), fill, np.uint8))
        d_rows = hip.upload(rows); d_a = pre(B * kmax * 8); d_rec = pre(B * _abi.RANSAC_RECORD_NBYTES)
        d_cnt = pre(B * ITER * 4) if counts else None
        d_T, d_n, d_s = pre(B * 128), pre(B * 4), pre(B * 4)
        d_lrec, d_idx, d_acc = pre(B * _abi.LC_RECORD_NBYTES), pre(B * 4), pre(4)
        if packed_call:
            ctx.ransac_batch_dev(rp, d_rows, off1, n1, off2, n2, kmax, d_a, d_rec, counts_out_ptr=d_cnt)
        else:
            kw = {}
            if lc is not None:
                T_ref, enable, FL, iL, FR, iR = lc.arrays(B)
                up = lambda a: None if a is None else hip.upload(a)
                kw = dict(lc_params=lc.params(), records_ptr=d_lrec, accepted_idx_ptr=d_idx, n_accepted_ptr=d_acc, T_ref_ptr=up(T_ref), enable_ptr=up(enable),
                          FL_ptr=up(FL), iL_ptr=up(iL), FR_ptr=up(FR), iR_ptr=up(iR))
            ctx.ransac_lc_batch_dev(rp, d_rows, F, off1, n1, off2, n2, kmax, d_a, d_rec, T_out_ptr=d_T, n_assoc_out_ptr=d_n, status_out_ptr=d_s,
                                    counts_out_ptr=d_cnt, **kw)
        ctx.sync()
        out = dict(rec=hip.download(d_rec, (B,), ransac_record_dtype()), assoc=hip.download(d_a, (B, kmax, 2), np.int32),
                   counts=hip.download(d_cnt, (B, ITER), np.int32) if counts else None,
                   T=hip.download(d_T, (B, 16), np.float64), n=hip.download(d_n, (B,), np.int32), status=hip.download(d_s, (B,), np.int32),
                   lrec=hip.download(d_lrec, (B,), lc_record_dtype()), idx=hip.download(d_idx, (B,), np.int32), acc=hip.download(d_acc, (1,), np.int32))
        if lc is not None:                                          # the tail on its own over the split outputs the call left on the device
            d_lrec2, d_idx2, d_acc2 = pre(B * _abi.LC_RECORD_NBYTES), pre(B * 4), pre(4)
            ctx.lc_tail_dev(kw["lc_params"], B, d_T, d_n, d_s, d_lrec2, d_idx2, d_acc2, **{k: v for k, v in kw.items() if k.endswith("_ptr") and k[:2] in ("T_", "en", "FL", "iL", "FR", "iR")})
            ctx.sync()
            out.update(lrec2=hip.download(d_lrec2, (B,), lc_record_dtype()), idx2=hip.download(d_idx2, (B,), np.int32), acc2=hip.download(d_acc2, (1,), np.int32))
        return out
    finally:
        hip.free_all()


@pytest.fixture(scope="module")
def runs(ctx):
    """The same 11 problems as packed rows, as wide rows whose other columns are NaN, and through roman_ransac_batch_dev."""
    assert _oracle_is_clean()
    pts, off1, n1, off2, n2 = _problems()
    kmax = int(np.max(n1.astype(np.int64) * n2))
    return dict(packed=run_dev(ctx, pts, off1, n1, off2, n2, kmax, counts=True), wide=run_dev(ctx, _wide(pts), off1, n1, off2, n2, kmax, counts=True),
                old=run_dev(ctx, pts, off1, n1, off2, n2, kmax, counts=True, packed_call=True), kmax=kmax)


def test_stride(runs):
    a, w, o = runs["packed"], runs["wide"], runs["old"]
    for k in ("rec", "assoc", "counts"):
        assert a[k].tobytes() == w[k].tobytes(), f"{k}: wide rows differ from packed rows"
        assert a[k].tobytes() == o[k].tobytes(), f"{k}: roman_ransac_lc_batch_dev differs from roman_ransac_batch_dev"
    ok = a["rec"]["status"] == _abi.ROMAN_ST_OK
    assert ok.sum() >= 6 and not np.isnan(a["rec"]["T"][ok]).any(), "a NaN column reached an OK pose"
    assert a["rec"]["n_assoc"][4] == 6                              # a map against itself
    # every processed hypothesis of every problem against the oracle — at n = 70 and n = 90 too, where scoring reads every staged point
    for b, want in _oracle_is_clean().items():
        assert a["rec"]["n_hyp"][b] == want.n_hyp and a["rec"]["n_scored"][b] == want.n_scored, b
        assert np.array_equal(a["counts"][b, :want.n_hyp], want.counts), b
    assert all(_oracle_is_clean()[b].n_scored >= 30 for b in (8, 9))
    # roman_ransac_batch_dev takes no split outputs: they stay as they were
    assert np.all(o["T"].view(np.uint8) == 0xAB) and np.all(o["n"].view(np.uint8) == 0xAB)


def test_split_outputs(ctx, runs, orc):
    pts, off1, n1, off2, n2 = _problems()
    for name in ("packed", "wide"):
        r = runs[name]
        assert r["T"].tobytes() == np.ascontiguousarray(r["rec"]["T"]).tobytes()
        assert np.array_equal(r["n"], r["rec"]["n_assoc"]) and np.array_equal(r["status"], r["rec"]["status"])
    st, rec = runs["packed"]["status"], runs["packed"]["rec"]
    assert st[5] == st[6] == _abi.ROMAN_ST_EMPTY_MAP and st[7] == _abi.ROMAN_ST_INSUFFICIENT and rec["best_hyp"][7] == -1 and rec["n_scored"][7] == 0
    assert np.isnan(runs["packed"]["T"][[5, 6, 7]]).all() and np.all(runs["packed"]["n"][[5, 6, 7]] == 0)
    # a small kmax: truncated rows, the FULL count and the pose of the full set in record and split outputs alike
    t = run_dev(ctx, pts, off1, n1, off2, n2, 3)
    trunc = (t["status"] & _abi.ROMAN_ST_ASSOC_TRUNCATED) != 0
    assert trunc.sum() >= 4 and np.array_equal(trunc, rec["n_assoc"] > 3)
    assert np.array_equal(t["n"], rec["n_assoc"]) and t["T"].tobytes() == runs["packed"]["T"].tobytes()
    assert np.array_equal(t["status"], t["rec"]["status"]) and np.array_equal(t["n"], t["rec"]["n_assoc"]) and t["T"].tobytes() == np.ascontiguousarray(t["rec"]["T"]).tobytes()
    # fewer than 3 inliers: a survivor, but nothing within a tenth of a millimetre of it
    P, Q, _, _, _ = ro.planted(6, 5, 105, n_in=4, noise=0.01)
    tiny = dict(max_dist=1e-4)
    want = ro.run(P, Q, max_iteration=ITER, round=ROUND, edge_len=EDGE, **tiny)
    assert want.n_border == 0 and want.n_scored > 0 and want.best_count < 3
    f = run_dev(ctx, np.vstack([P, Q]), np.array([0], np.int64), np.array([6], np.int32), np.array([6], np.int64), np.array([5], np.int32), 30, rp=_params(**tiny))
    assert f["status"][0] == f["rec"]["status"][0] == _abi.ROMAN_ST_INSUFFICIENT and f["rec"]["best_hyp"][0] >= 0 and f["rec"]["n_scored"][0] == want.n_scored
    assert f["n"][0] == f["rec"]["n_assoc"][0] == want.best_count and np.isnan(f["T"][0]).all() and np.isnan(f["rec"]["T"][0]).all()


def _lc(B, seed, **kw):
    rng = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation as Rot

    def frames(n):
        T = np.tile(np.eye(4), (n, 1, 1)); T[:, :3, :3] = Rot.random(n, random_state=seed + n).as_matrix(); T[:, :3, 3] = rng.uniform(-5, 5, (n, 3))
        return T
    opt = dict(T_ref=frames(B), enable=(np.arange(B) % 3 != 1).astype(np.int32), FL=frames(3), iL=rng.integers(0, 3, B), FR=frames(4), iR=rng.integers(0, 4, B))
    return LcInputs(dim=3, lc_association_thresh=4, **{**opt, **kw})


@pytest.mark.parametrize("name", ["everything-rm-roll-pitch", "upside-down-bare", "tilt"])
def test_tail(ctx, runs, name):
    pts, off1, n1, off2, n2 = _problems()
    B = len(n1)
    lc = {"everything-rm-roll-pitch": lambda: _lc(B, 5, force_rm_lc_roll_pitch=True),
          "upside-down-bare": lambda: LcInputs(dim=3, lc_association_thresh=4, force_rm_upside_down=True),
          "tilt": lambda: _lc(B, 6, tilt_thresh=0.3, FL=None, iL=None)}[name]()
    r = run_dev(ctx, _wide(pts), off1, n1, off2, n2, runs["kmax"], lc=lc)
    assert r["rec"].tobytes() == runs["packed"]["rec"].tobytes() and r["assoc"].tobytes() == runs["packed"]["assoc"].tobytes()
    # the fused tail is roman_lc_tail_dev over the split outputs, to the byte
    assert r["lrec"].tobytes() == r["lrec2"].tobytes() and r["acc"][0] == r["acc2"][0]
    k = int(r["acc"][0])
    assert np.array_equal(r["idx"][:k], r["idx2"][:k]) and np.all(np.diff(r["idx"][:k]) > 0)
    want, want_acc = lt.lc_tail(lc, r["T"].reshape(B, 4, 4), r["n"], r["status"])
    lt.assert_records_match(r["lrec"], r["idx"][:k], want, want_acc)
    fl = r["lrec"]["flags"]
    assert np.all(fl[[5, 6, 7]] == _abi.ROMAN_LC_FAILED_INSUFFICIENT) and (k >= 2 or name == "tilt")     # (random attitudes: the tilt check leaves none)
    if name == "everything-rm-roll-pitch":
        assert ((r["n"] >= 4) & (lc.enable == 0) & ((fl & _abi.ROMAN_LC_ACCEPTED) == 0)).any(), "enable stopped no pair with enough associations"
        acc = r["idx"][:k]
        assert np.allclose(r["lrec"]["T_hat"][acc][:, 2, :3], [0, 0, 1]) and not np.isnan(r["lrec"]["theta"][acc]).any()
    if name == "upside-down-bare":
        assert np.isnan(r["lrec"]["theta"][fl == _abi.ROMAN_LC_ACCEPTED]).all()         # no reference transform
    if name == "tilt":
        assert (fl == _abi.ROMAN_LC_FAILED_TILT).any()
    # without lc_params the records buffer is untouched
    assert np.all(runs["wide"]["lrec"].view(np.uint8) == 0xAB) and np.all(runs["wide"]["acc"].view(np.uint8) == 0xAB)


def test_host_pointer_form(ctx, runs):
    pts, off1, n1, off2, n2 = _problems()
    B = len(n1)
    lc = _lc(B, 5, force_rm_lc_roll_pitch=True)
    dev = run_dev(ctx, _wide(pts), off1, n1, off2, n2, runs["kmax"], lc=lc)
    saved = ctx.host_batching
    try:
        for chunk in (saved[0], 4):                                 # one call; B = 11 in calls of 4, 4 and 3 with one tail behind them
            ctx.set_host_batching(chunk, saved[1])
            res = ctx.ransac_lc_batch(_params(), _wide(pts), off1, n1, off2, n2, lc, kmax=runs["kmax"], counts=True)
            assert res.ransac_records.tobytes() == dev["rec"].tobytes(), chunk
            assert res.records.tobytes() == dev["lrec"].tobytes() and np.array_equal(res.accepted, dev["idx"][:int(dev["acc"][0])])
            assert res.T.tobytes() == dev["T"].tobytes() and np.array_equal(res.status, dev["status"])
            assert all(np.array_equal(res.assoc[b], dev["assoc"][b, :dev["n"][b]]) for b in range(B))
            assert np.all(res.stats["n_pass"] == 0)
    finally:
        ctx.set_host_batching(*saved)
    # the packed host call is the F = 3 case of the same code
    old = ctx.ransac_batch(_params(), pts, off1, n1, off2, n2, kmax=runs["kmax"])
    assert old.records.tobytes() == dev["rec"].tobytes()
    empty = ctx.ransac_lc_batch(_params(), np.zeros((0, 5)), [], [], [], [], LcInputs(dim=3))
    assert len(empty.accepted) == 0 and len(empty.records) == 0


def test_validation(ctx, runs):
    """Every refusal happens on the host, in front of any enqueue: the pointers handed in are real buffers all the same."""
    pts, off1, n1, off2, n2 = _problems()
    B = len(n1)
    hip = Hip()
    try:
        d_rows = hip.upload(_wide(pts)); buf = [hip.alloc(B * runs["kmax"] * 8) for _ in range(9)]
        d_a, d_rec, d_T, d_n, d_s, d_lrec, d_idx, d_acc, d_x = buf
        lp = LcInputs(dim=3).params()

        def call(code, rp=None, F=WIDE, kmax=None, n1_=n1, **kw):
            args = dict(T_out_ptr=d_T, n_assoc_out_ptr=d_n, status_out_ptr=d_s, lc_params=lp, records_ptr=d_lrec, accepted_idx_ptr=d_idx, n_accepted_ptr=d_acc)
            args.update(kw)
            with pytest.raises(RomanHipError) as e:
                ctx.ransac_lc_batch_dev(rp or _params(), d_rows, F, off1, n1_, off2, n2, runs["kmax"] if kmax is None else kmax, d_a, d_rec, **args)
            assert e.value.code == code and str(e.value).split(":", 1)[1].strip(), e.value
        E = _abi.ROMAN_E_INVALID
        call(E, rp=_params(max_iteration=0)); call(E, rp=_params(round=0)); call(E, rp=_params(edge_len=1.5)); call(E, rp=_params(max_dist=0.0))
        call(E, rp=_params(confidence=1.0)); call(E, kmax=-1); call(E, n1_=-n1)
        call(E, F=2)
        call(E, T_out_ptr=None); call(E, n_assoc_out_ptr=None); call(E, status_out_ptr=None)
        call(E, lc_params=LcInputs(dim=2).params())
        bad = LcInputs(dim=3).params(); bad.reserved[1] = 1
        call(E, lc_params=bad)
        call(E, FL_ptr=d_x); call(E, iL_ptr=d_x); call(E, FR_ptr=d_x); call(E, iR_ptr=d_x)
        call(E, n_accepted_ptr=None); call(E, records_ptr=None)
        big = n1.copy(); big[0] = _abi.ROMAN_RANSAC_MAX_OBJECTS + 1
        call(_abi.ROMAN_E_TOO_LARGE, n1_=big)
        with pytest.raises(ValueError):
            ctx.ransac_lc_batch(_params(), np.zeros((4, 2)), [0], [2], [2], [2], LcInputs(dim=3))
        # B = 0 with a tail writes n_accepted = 0
        e64, e32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        ctx.ransac_lc_batch_dev(_params(), None, 3, e64, e32, e64, e32, 1, None, None, lc_params=lp, n_accepted_ptr=d_acc)
        ctx.sync()
        assert hip.download(d_acc, (1,), np.int32)[0] == 0
    finally:
        hip.free_all()
    # the context still runs a good call
    again = run_dev(ctx, pts, off1, n1, off2, n2, runs["kmax"])
    assert again["rec"].tobytes() == runs["packed"]["rec"].tobytes()


def _compare_end_to_end(got, want, subs):
    assert np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
    n0, n1 = want.clipper_num_associations.shape
    for i in range(n0):
        for j in range(n1):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
    for name in ("robots_nearby_mat", "T_ij_mat", "T_ij_hat_mat", "submap_yaw_diff_mat", "clipper_angle_mat", "clipper_dist_mat"):
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True, err_msg=name)
    if want.similarity_mat is not None:
        np.testing.assert_allclose(got.similarity_mat, want.similarity_mat, rtol=0, atol=1e-9, equal_nan=True)
    rl.assert_same_edges(got, want, subs, atol=1e-9)


@pytest.mark.parametrize("kind", ["mean-semantic-over-roman-pool", "self-shared-ids"])
def test_end_to_end(ctx, orc, kind, monkeypatch):
    dev = f"cuda:{ctx.device}"
    if kind == "self-shared-ids":
        p, io, (pools, segs) = cpu._config(kind, None, self_pool=cpu._self_pool(ctx, dev))
    else:
        p, io, (pools, segs) = cpu._config(kind, {"roman": cpu._build("roman", 'mean_semantic', ctx=ctx, device=dev)})
    reg = cpu._ransac_reg(ctx)
    got = sa.submap_align_pools(p, pools, io, registration=reg)
    want, subs = cpu._pair_loop(orc, p, io, pools, segs)           # (the oracle double asserts: no borderline hypothesis, no tie)
    print(kind, "pairs registered:", len(got.timing_list), "\n", want.clipper_num_associations)
    _compare_end_to_end(got, want, subs)
    assert (want.clipper_num_associations >= cpu.THRESH).sum() >= 2 and len(got.lc_edges["pairs"]) >= 1
    assert int(pools[0].pool.shape[1]) == (WIDE if kind.startswith("mean") else 3)
    # two chunks: the same results, to the bit
    B = len(got.timing_list)
    kmax = int(max(q.count.max() for q in pools)) ** 2
    monkeypatch.setattr(sa, "RANSAC_ASSOC_CHUNK_BYTES", 8 * kmax * -(-B // 2))
    two = sa.submap_align_pools(p, pools, io, registration=reg)
    cpu._all_equal(two, got)
