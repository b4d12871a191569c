"""The pair loop is really gone from the grid form: the number of Python-level calls into
scipy.spatial.transform.Rotation during submap_align_grid() does not grow with the number of PAIRS."""
import numpy as np

import _lc_tail as lt
from roman_amd import synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.runtime import BatchResult, stats_dtype


class CountingRot:
    """Stands in for the module's `Rot`: forwards to scipy and counts every call."""
    calls = 0

    @classmethod
    def _fwd(cls, name):
        from scipy.spatial.transform import Rotation
        def f(*a, **k):
            cls.calls += 1
            return getattr(Rotation, name)(*a, **k)
        return f


for _n in ("from_matrix", "from_euler", "from_quat", "from_rotvec", "identity", "random"):
    setattr(CountingRot, _n, staticmethod(CountingRot._fwd(_n)))


def grid_submaps(S, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(2):
        rob = []
        for k in range(S):
            pose = synth.yaw_transform(rng.uniform(-3, 3), rng.uniform(-4, 4, 3), roll=rng.normal(0, 0.03), pitch=rng.normal(0, 0.03))
            gt = pose @ synth.yaw_transform(rng.normal(0, 0.05), rng.normal(0, 0.2, 3))
            rob.append(sa.Submap(id=k, time=500.0 * r + 7.0 * k, segments=[lt._Seg(1000 * r + 10 * k + q) for q in range(4)], pose_flu=pose, pose_flu_gt=gt))
        out.append(rob)
    return out


def recording_compute(calls):
    def compute(registration, batch, lc):
        B = len(batch); calls.append(B)
        rng = np.random.default_rng(B)
        T = np.tile(np.eye(4), (B, 1, 1)); T[:, :3, 3] = rng.uniform(-2, 2, (B, 3))
        assoc = [np.zeros((int(k), 2), np.int32) for k in rng.integers(0, 12, B)]
        return lt.as_lc_result(BatchResult(assoc, T, np.zeros(B, np.int32), np.zeros(B, stats_dtype())), lc)
    return compute


def count_calls(S, monkeypatch, fn, gt_available):
    monkeypatch.setattr(sa, "Rot", CountingRot)
    CountingRot.calls = 0
    submaps = grid_submaps(S, 3)
    calls = []
    p = SubmapAlignParams(submap_radius=1e3)
    io = sa.SubmapAlignIO(lc_association_thresh=4, gt_available=gt_available)
    reg = lt.StubRegistration(3, False)
    if fn is sa.submap_align_grid:
        res = fn(p, submaps, io, registration=reg, compute=recording_compute(calls))
    else:
        lc_calls = recording_compute(calls)
        res = fn(p, submaps, io, registration=reg, compute=lambda r, b: lc_calls(r, b, lt.LcInputs(T_ref=np.tile(np.eye(4), (len(b), 1, 1)))))
    edges = sa.loop_closure_edges(res, submaps)
    assert calls == [S * S] and len(edges) > S           # one batched call over every pair; plenty of loop closures
    return CountingRot.calls


def test_rotation_calls_do_not_grow_with_the_pairs(monkeypatch):
    """S0 = S1 = 24: 576 pairs.  Per SUBMAP the grid form needs: reading the gravity-aligned pose until it is a fixed point (pass
    1: at most 3 reads of 2 Rotation calls each for a pose that settles after two, for the odometry OR the ground-truth pose),
    one read for the submap's edge frames (2 calls), and the reads loop_closure_edges() owes the caller's submaps (again at most
    3 x 2) — 14 calls; the bound is 16 per submap.  The pair loop makes more than 4 per PAIR."""
    S = 24
    for gt in ((False, False), (True, True)):
        n_grid = count_calls(S, monkeypatch, sa.submap_align_grid, gt)
        assert n_grid <= 16 * (S + S), n_grid
        n_half = count_calls(S // 2, monkeypatch, sa.submap_align_grid, gt)
        assert n_half <= 16 * S, n_half                      # the same bound per submap at a quarter of the pairs
    n_loop = count_calls(S, monkeypatch, sa.submap_align, (False, False))
    assert n_loop > 4 * S * S                                # the yardstick really counts: the existing pair loop pays per pair
