"""roman_ransac_batch on the device against the NumPy oracle of DESIGN.md §4.7 (tests/_ransac_oracle.py).

The device's Kabsch fit and NumPy's differ by rounding, so counts can only be compared exactly away from the thresholds: every
case here has ZERO borderline hypotheses under the oracle (asserted), found on the CPU beforehand.  Tolerances: counts, flags and
indices are exact; sums of squared distances 1e-9 relative (a few hundred f64 additions in another order, and fits that differ in
the last bits); poses 1e-12 in the Frobenius norm."""
import functools

import numpy as np
import pytest

import _ransac_oracle as ro
from roman_amd import _abi, synth
from roman_amd.align import RansacReg, SubmapAlignParams
from roman_amd.align.submap_align import Submap, submap_align, submap_align_grid
from roman_amd.runtime import RomanHipError

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-12
SSE_RTOL = 1e-9
SENTINEL = -2                                                   # what Context.ransac_batch(counts=True) pre-fills

# (n, m, point seed, parameter overrides).  The first four are the shapes every hypothesis is checked at with the defaults
# (max_iteration 2048, round 256, edge_len 0.95: a random triple rarely passes the edge test, so few hypotheses are scored).  The
# last two lower edge_len so that a third of the hypotheses survive, with rounds long enough that a wave's queue fills (512 and
# 250 hypotheses per wave and round: the full-queue path and the masked flush), and a round length that is no multiple of 256.
CASES = {
    "3x3": (3, 3, 100, {}),
    "4x7": (4, 7, 101, {}),
    "12x9": (12, 9, 100, {}),
    "40x40": (40, 40, 100, {}),
    "40x40-loose": (40, 40, 100, dict(edge_len=0.5, round=2048)),
    "33x21-loose": (33, 21, 102, dict(edge_len=0.5, round=1000)),
}
DEFAULTS = dict(max_iteration=2048, round=256, edge_len=0.95, max_dist=0.5, confidence=0.999, seed=0)


def _params(**kw):
    k = dict(DEFAULTS, **kw)
    return _abi.RomanRansacParams(k["max_iteration"], k["round"], k["edge_len"], k["max_dist"], k["confidence"], k["seed"])


def _points(name):
    n, m, seed, _ = CASES[name]
    P, Q, _, _, _ = ro.planted(n, m, seed, n_in=max(3, int(0.6 * min(n, m))))
    return P, Q


@functools.lru_cache(maxsize=None)
def _oracle(name):
    P, Q = _points(name)
    res = ro.run(P, Q, **dict(DEFAULTS, **CASES[name][3]))
    assert res.n_border == 0, "the case must stay away from the thresholds"
    return res


def _single(ctx, P, Q, counts=True, kmax=None, **kw):
    return ctx.ransac_batch(_params(**kw), np.vstack([P, Q]), [0], [len(P)], [len(P)], [len(Q)], kmax=kmax, counts=counts)


_DEVICE = {}


def _device(ctx, name):
    if name not in _DEVICE:
        P, Q = _points(name)
        _DEVICE[name] = _single(ctx, P, Q, **CASES[name][3])
    return _DEVICE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_hypothesis(ctx, name):
    """Sampler, both prune rules, the Kabsch call, the inlier test and the round loop in one comparison."""
    want, got = _oracle(name), _device(ctx, name)
    rec = got.records[0]
    print(f"{name}: n_hyp {rec['n_hyp']} (oracle {want.n_hyp}), n_scored {rec['n_scored']} ({want.n_scored}), best_count {rec['best_count']} ({want.best_count})")
    assert rec["n_hyp"] == want.n_hyp and rec["n_scored"] == want.n_scored and rec["best_count"] == want.best_count
    assert np.array_equal(got.counts[0, :want.n_hyp], want.counts)
    assert np.all(got.counts[0, want.n_hyp:] == SENTINEL)
    if name.endswith("loose"):
        assert want.n_scored > 256                               # these cases are here for the full queues


@pytest.mark.parametrize("name", list(CASES))
def test_winner(ctx, orc, name):
    want, got = _oracle(name), _device(ctx, name)
    rec = got.records[0]
    assert want.best_set and ro.same_triple(want, want.best_set)          # a singleton, or copies of one triple
    assert int(rec["best_hyp"]) in want.best_set
    rows, sse = ro.inlier_rows(want, int(rec["best_hyp"]))
    print(f"{name}: best_hyp {rec['best_hyp']} of {want.best_set}, {len(rows)} rows, sse {rec['best_sse']:.15g} (oracle {sse:.15g})")
    assert rec["n_assoc"] == len(rows) and np.array_equal(got.assoc[0], rows)
    assert abs(rec["best_sse"] - sse) <= SSE_RTOL * sse
    assert got.status[0] == _abi.ROMAN_ST_OK and rec["status"] == _abi.ROMAN_ST_OK
    err = np.linalg.norm(got.T[0] - ro.pose_on(orc, want.P, want.Q, rows))
    print(f"  |T - T_oracle|_F = {err:.3e}")
    assert err < POSE_TOL


def test_early_stop(ctx):
    """The CPU stop case: n = m = 4, all planted, rounds of 64."""
    P, Q, _, _, _ = ro.planted(4, 4, 201)
    want = ro.run(P, Q, max_iteration=4096, round=64)
    assert want.n_border == 0 and want.n_hyp == 448
    got = _single(ctx, P, Q, max_iteration=4096, round=64)
    assert got.records["n_hyp"][0] == want.n_hyp and got.records["best_count"][0] == 4
    assert np.array_equal(got.counts[0, :want.n_hyp], want.counts)
    assert np.all(got.counts[0, want.n_hyp:] == SENTINEL)        # nothing written beyond n_hyp


def test_cut_round(ctx):
    P, Q = _points("12x9")
    want = ro.run(P, Q, **dict(DEFAULTS, max_iteration=300))
    assert want.n_border == 0 and want.n_hyp == 300
    got = _single(ctx, P, Q, max_iteration=300)
    assert got.records["n_hyp"][0] == 300 and got.counts.shape == (1, 300)
    assert np.array_equal(got.counts[0], want.counts) and got.records["n_scored"][0] == want.n_scored


def test_nothing_survives(ctx):
    """Map 2 is map 1 scaled by 2: every triple fails the edge test."""
    P, _ = _points("12x9")
    Q = 2.0 * P
    want = ro.run(P, Q, **DEFAULTS)
    assert want.n_border == 0 and want.n_scored == 0
    got = _single(ctx, P, Q)
    rec = got.records[0]
    assert rec["n_hyp"] == 2048 and rec["n_scored"] == 0 and rec["best_hyp"] == -1 and rec["n_assoc"] == 0
    assert got.assoc[0].shape == (0, 2) and np.all(np.isnan(got.T[0])) and got.status[0] == _abi.ROMAN_ST_INSUFFICIENT
    assert np.all(got.counts[0] == -1)
    reg = RansacReg(max_iteration=2048, round=256); reg.set_context(ctx)
    out = reg.register(ro.segments(P), ro.segments(Q))
    assert out.shape == (0, 2) and np.issubdtype(out.dtype, np.integer)


def test_edges_of_the_interface(ctx, orc):
    P, Q = _points("40x40-loose")
    loose = CASES["40x40-loose"][3]
    # an empty map
    got = ctx.ransac_batch(_params(), P, [0, 0], [0, 5], [0, 0], [5, 0], counts=True)
    assert np.all(got.status == _abi.ROMAN_ST_EMPTY_MAP) and np.all(np.isnan(got.T)) and all(a.shape == (0, 2) for a in got.assoc)
    assert np.all(got.records["n_hyp"] == 0) and np.all(got.records["best_hyp"] == -1) and np.all(got.counts == SENTINEL)
    # a side above the cap; the context stays usable
    big = np.zeros((1025 + 3, 3))
    with pytest.raises(RomanHipError) as e:
        ctx.ransac_batch(_params(), big, [0], [1025], [1025], [3])
    assert e.value.code == _abi.ROMAN_E_TOO_LARGE
    with pytest.raises(RomanHipError) as e:
        ctx.ransac_batch(_params(), big, [1025], [3], [0], [1025])
    assert e.value.code == _abi.ROMAN_E_TOO_LARGE
    want, full = _oracle("40x40-loose"), _device(ctx, "40x40-loose")
    again = _single(ctx, P, Q, **loose)
    assert np.array_equal(again.counts, full.counts) and again.records.tobytes() == full.records.tobytes()
    # kmax below the inlier count: the first kmax rows, count / key / pose from the full set
    assert full.records["n_assoc"][0] == 6
    cut = _single(ctx, P, Q, kmax=4, **loose)
    assert cut.status[0] == _abi.ROMAN_ST_ASSOC_TRUNCATED and cut.records["n_assoc"][0] == 6
    assert np.array_equal(cut.assoc[0], full.assoc[0][:4])
    assert np.array_equal(cut.T[0], full.T[0]) and cut.records["best_sse"][0] == full.records["best_sse"][0]
    rows, _ = ro.inlier_rows(want, int(cut.records["best_hyp"][0]))
    assert np.linalg.norm(cut.T[0] - ro.pose_on(orc, P, Q, rows)) < POSE_TOL
    # each invalid parameter
    for bad in (dict(max_iteration=0), dict(round=0), dict(edge_len=0.0), dict(edge_len=1.5), dict(max_dist=0.0), dict(max_dist=-1.0),
                dict(confidence=0.0), dict(confidence=1.0)):
        with pytest.raises(RomanHipError) as e:
            _single(ctx, P, Q, counts=None, **bad)
        assert e.value.code == _abi.ROMAN_E_INVALID, bad
    assert _single(ctx, P, Q, counts=None, edge_len=1.0, max_iteration=64, round=64).records["n_hyp"][0] == 64     # the closed end of (0, 1]


def test_batch_equals_singles_twice(ctx):
    names = ["12x9", "3x3", "40x40-loose", "4x7", "33x21-loose"]
    kw = dict(edge_len=0.5, round=512)
    pts, off1, n1, off2, n2 = [], [], [], [], []
    at = 0
    for nm in names:
        P, Q = _points(nm)
        off1.append(at); n1.append(len(P)); off2.append(at + len(P)); n2.append(len(Q)); at += len(P) + len(Q)
        pts += [P, Q]
    pts = np.vstack(pts)
    one = ctx.ransac_batch(_params(**kw), pts, off1, n1, off2, n2, counts=True)
    for b, nm in enumerate(names):
        P, Q = _points(nm)
        s = _single(ctx, P, Q, **kw)
        assert np.array_equal(one.counts[b], s.counts[0]), nm
        assert one.records[b].tobytes() == s.records[0].tobytes(), nm
        assert np.array_equal(one.assoc[b], s.assoc[0]) and np.array_equal(one.T[b], s.T[0], equal_nan=True), nm
    two = ctx.ransac_batch(_params(**kw), pts, off1, n1, off2, n2, counts=True)
    assert two.counts.tobytes() == one.counts.tobytes() and two.records.tobytes() == one.records.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(one.assoc, two.assoc)) and two.T.tobytes() == one.T.tobytes()
    other = ctx.ransac_batch(_params(seed=1, **kw), pts, off1, n1, off2, n2, counts=True)
    assert not np.array_equal(other.counts, one.counts)


def _grid_scenario(seed=9003):
    """Two robots with three submaps of 8 objects each (5 shared landmarks, 1 cm noise); one submap is empty."""
    subs, poses = synth.make_submap_grid(6, n=8, d=0, seed0=seed, overlap=0.625, noise=0.01)
    return [[Submap(id=k, time=100.0 * r + 30.0 * k, segments=([] if (r, k) == (1, 1) else subs[3 * r + k]), pose_flu=poses[3 * r + k].copy())
             for k in range(3)] for r in range(2)]


def test_through_the_plugin(ctx, orc):
    sm = SubmapAlignParams(method='ransac', ransac_iter=2048)
    reg = sm.get_object_registration(); reg.set_context(ctx)
    got = submap_align(sm, _grid_scenario(), registration=reg)
    want = submap_align(SubmapAlignParams(method='ransac', ransac_iter=2048), _grid_scenario(), compute=ro.compute_double(orc))
    print(got.clipper_num_associations)
    assert np.array_equal(got.clipper_num_associations, want.clipper_num_associations)
    assert np.array_equal(got.robots_nearby_mat, want.robots_nearby_mat, equal_nan=True)
    assert len(set(got.clipper_num_associations.ravel().tolist())) >= 3      # found, junk and nothing all occur
    for i in range(3):
        for j in range(3):
            assert np.array_equal(np.asarray(got.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(want.associated_objs_mat[i][j]).reshape(-1, 2)), (i, j)
            a, b = got.T_ij_hat_mat[i, j], want.T_ij_hat_mat[i, j]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (i, j)
            if not np.isnan(b).any():
                assert np.linalg.norm(a - b) < POSE_TOL, (i, j)
    for name in ("clipper_angle_mat", "clipper_dist_mat"):
        assert np.allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-9, equal_nan=True), name
    with pytest.raises(NotImplementedError):
        submap_align_grid(sm, _grid_scenario(), registration=reg)
