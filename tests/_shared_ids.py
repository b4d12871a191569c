"""The shared-segment removal of self loop closures, stated twice — TEST INFRASTRUCTURE.

`reference_wording()` says it the way the reference does ([REF roman/align/submap_align.py:108-115]): Python sets over `seg.id`,
their intersection, list comprehensions.  `mark()` is the NumPy model of the device's mark step (k_shared_mark) in the layout of
the C ABI (roman_shared_ids_dev): per problem and side the ascending local indices that stay, and their count.
tests/test_shared_ids_cpu.py ties the two together; the GPU tests compare the device with `mark()`.

`edge_batch()` is the batch of awkward problems both tests use, `reduce_on_host()` today's 2 B pool built from the kept lists,
and `StubIdsContext` a stand-in for runtime.Context on a box without a GPU: `align_lc_batch_ids` computed with `mark()`, the
CPU oracle and the NumPy tail (tests/_lc_tail.py)."""
import numpy as np

import _lc_tail as lt

TILE = 1024          # ids of the other side the kernel stages in LDS at a time (SHARE_TILE in roman_amd/csrc/kernels.hip.h)


class Seg:
    def __init__(self, id):
        self.id = id


def reference_wording(ids_i, ids_j):
    """-> (kept local indices of side i, of side j) through sets and list comprehensions over segment objects."""
    segs_i, segs_j = [Seg(v) for v in ids_i], [Seg(v) for v in ids_j]
    common = {seg.id for seg in segs_i} & {seg.id for seg in segs_j}
    keep_i = [k for k, s in enumerate(segs_i) if s.id not in common]
    keep_j = [k for k, s in enumerate(segs_j) if s.id not in common]
    return keep_i, keep_j


def mark(ids, off1, n1, off2, n2):
    """-> (keep int32[sum(n1 + n2)], kept int32[B, 2]).  Problem b's side-1 list starts at sum over c < b of (n1[c] + n2[c]), its
    side-2 list n1[b] later; entries behind the kept count of a list are -1 (the device leaves them unwritten)."""
    ids = np.asarray(ids, dtype=np.int64)
    B = len(n1)
    keep = np.full(int(np.sum(n1, dtype=np.int64) + np.sum(n2, dtype=np.int64)), -1, dtype=np.int32)
    kept = np.zeros((B, 2), dtype=np.int32)
    base = 0
    for b in range(B):
        a = ids[off1[b]:off1[b] + n1[b]]; c = ids[off2[b]:off2[b] + n2[b]]
        k1 = np.nonzero(~np.isin(a, c))[0]; k2 = np.nonzero(~np.isin(c, a))[0]
        keep[base:base + len(k1)] = k1; keep[base + n1[b]:base + n1[b] + len(k2)] = k2
        kept[b] = (len(k1), len(k2))
        base += int(n1[b]) + int(n2[b])
    return keep, kept


def kept_lists(keep, kept, n1, n2):
    """The (side-1, side-2) kept index arrays of every problem out of the ABI layout."""
    out, base = [], 0
    for b in range(len(n1)):
        out.append((keep[base:base + kept[b, 0]], keep[base + n1[b]:base + n1[b] + kept[b, 1]]))
        base += int(n1[b]) + int(n2[b])
    return out


def compare_written(got_keep, got_kept, want_keep, want_kept, n1, n2):
    """Counts equal, and every list equal in its first `kept` entries (what lies behind them is not specified)."""
    np.testing.assert_array_equal(got_kept, want_kept)
    for b, ((g1, g2), (w1, w2)) in enumerate(zip(kept_lists(got_keep, got_kept, n1, n2), kept_lists(want_keep, want_kept, n1, n2))):
        assert np.array_equal(g1, w1) and np.array_equal(g2, w2), b


def edge_batch(seed=0):
    """-> (ids int64[n_objects], off1, n1, off2, n2, names): one pool and the problems over it that the mark step can get wrong.
    Sizes straddle one wave (64), one workgroup (256) and one LDS tile (TILE = 1024: the pair (1030, 70) has 1030 ids on the
    OTHER side of its side 2 — two tiles — and five own chunks of 256 on its side 1)."""
    rng = np.random.default_rng(seed)
    pool, probs, names = [], [], []

    def add(a):
        o = sum(len(x) for x in pool); pool.append(np.asarray(a, dtype=np.int64)); return o, len(a)

    def problem(name, a, c):
        (o1, m1), (o2, m2) = add(a), add(c)
        probs.append((o1, m1, o2, m2)); names.append(name)

    def overlapping(m1, m2, share):
        u = rng.permutation(10 * (m1 + m2))[:m1 + m2 - share] + 1000
        a = u[:m1]; c = np.concatenate([u[:share], u[m1:]])
        return rng.permutation(a), rng.permutation(c)

    problem("n1 = 0", [], [5, 6, 7])
    problem("n2 = 0", [5, 6, 7], [])
    problem("both empty", [], [])
    problem("1 x 1 equal", [42], [42])
    problem("1 x 1 unequal", [42], [43])
    for (m1, m2) in ((63, 64), (64, 65), (65, 1), (257, 300), (1030, 70)):
        problem(f"{m1} x {m2}", *overlapping(m1, m2, min(m1, m2) // 3 + 1))
    problem("last id of a 1030 map only", np.arange(1030) + 10 ** 6, [10 ** 6 + 1029, 3, 4])      # found in the second tile, last slot
    problem("all shared", *overlapping(90, 90, 90))
    problem("none shared", *overlapping(70, 130, 0))
    hi = np.int64(1) << 32
    problem("equal low words, different high words", [7, 7 + hi, 9 + 2 * hi, 11], [7 + 2 * hi, 9, 11 + hi, 5])
    problem("equal low words, one really equal", [7 + hi, 8 + hi], [7, 8 + hi])
    problem("negative ids", [-1, -2, -(1 << 40), 3, -(2 ** 63)], [-2, 3, 1 << 40, -(2 ** 63), 1])
    problem("an id three times in one map, once in the other", [5, 9, 5, 7, 5, 8], [1, 5, 2])
    problem("an id three times in one map, absent from the other", [5, 9, 5, 7, 5, 8], [1, 9, 2])
    o, m = add(rng.permutation(100)[:77])
    probs.append((o, m, o, m)); names.append("the same submap on both sides")
    (oa, ma), (ob, mb), (oc, mc) = add(np.arange(50)), add(np.arange(40, 120)), add(np.arange(100, 130))
    probs.append((oa, ma, ob, mb)); names.append("shares its slice (1)")
    probs.append((ob, mb, oc, mc)); names.append("shares its slice (2)")
    ids = np.concatenate(pool) if pool else np.zeros(0, np.int64)
    P = np.array(probs, dtype=np.int64)
    return ids, P[:, 0].copy(), P[:, 1].astype(np.int32), P[:, 2].copy(), P[:, 3].astype(np.int32), names


def small_batch(seed=1):
    """Problems whose maps all have at most 64 objects: the call takes the one-wave-per-problem form of the kernel."""
    rng = np.random.default_rng(seed)
    pool, probs = [], []
    for m1, m2, lo in ((64, 64, 10), (1, 64, 0), (64, 1, 1), (33, 47, 20), (0, 12, 0), (20, 40, 7)):
        u = rng.permutation(1000)[:m1 + m2] - 500
        a, c = u[:m1], u[m1:].copy()
        k = min(lo, m1, m2); c[:k] = a[:k]
        o1 = sum(len(x) for x in pool); pool.append(a.astype(np.int64)); o2 = o1 + m1; pool.append(rng.permutation(c).astype(np.int64))
        probs.append((o1, m1, o2, m2))
    P = np.array(probs, dtype=np.int64)
    return np.concatenate(pool), P[:, 0].copy(), P[:, 1].astype(np.int32), P[:, 2].copy(), P[:, 3].astype(np.int32)


def reduce_on_host(feats, ids, off1, n1, off2, n2):
    """Today's per-pair form of the same batch: a pool of 2 B reduced maps built on the host from the model's kept lists
    -> (feats2, off1, n1, off2, n2, keep, kept)."""
    keep, kept = mark(ids, off1, n1, off2, n2)
    rows, offs = [], [0]
    for b, (k1, k2) in enumerate(kept_lists(keep, kept, n1, n2)):
        rows.append(feats[off1[b] + k1]); offs.append(offs[-1] + len(k1))
        rows.append(feats[off2[b] + k2]); offs.append(offs[-1] + len(k2))
    offs = np.array(offs, dtype=np.int64)
    f2 = np.concatenate(rows, axis=0) if rows else np.zeros((0, feats.shape[1]))
    return (np.ascontiguousarray(f2), offs[0:-1:2].copy(), kept[:, 0].copy(), offs[1::2].copy(), kept[:, 1].copy(), keep, kept)


class StubIdsContext:
    """Stands in for runtime.Context under submap_align_grid's default compute: `align_lc_batch_ids` through the NumPy model, the
    CPU oracle per problem and the NumPy tail; every call is recorded."""

    def __init__(self, registration):
        self.registration = registration
        self.calls = []                                  # (entry, problems, rows of the uploaded pool)

    def align_lc_batch_ids(self, params, feats, ids, off1, n1, off2, n2, lc, assoc=None, assoc_off=None, u0=None, kmax=None, want_keep=True):
        from roman_amd.align.batch import AlignmentBatch
        from test_submap_align import oracle_compute
        assert assoc is None and len(ids) == feats.shape[0]
        self.calls.append(("align_lc_batch_ids", len(n1), feats.shape[0]))
        f2, o1, m1, o2, m2, keep, kept = reduce_on_host(feats, ids, off1, n1, off2, n2)
        res = lt.as_lc_result(oracle_compute(self.registration, AlignmentBatch(f2, o1, m1, o2, m2)), lc)
        res.n1_kept, res.n2_kept, res.keep = kept[:, 0].copy(), kept[:, 1].copy(), keep if want_keep else None
        return res

    def align_lc_batch(self, params, feats, off1, n1, off2, n2, lc, assoc=None, assoc_off=None, u0=None, kmax=None):
        from roman_amd.align.batch import AlignmentBatch
        from test_submap_align import oracle_compute
        self.calls.append(("align_lc_batch", len(n1), feats.shape[0]))
        return lt.as_lc_result(oracle_compute(self.registration, AlignmentBatch(feats, off1, n1, off2, n2, assoc, assoc_off)), lc)
