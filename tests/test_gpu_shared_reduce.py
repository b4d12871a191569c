"""roman_shared_reduce_dev on the GPU (k_shared_reduce: mark and gather of a problem in one launch) against the
NumPy model of tests/_shared_ids.py and against roman_shared_ids_dev on the same call.

Every word of the feature rows is a distinct finite bit pattern, the gather region is pre-filled with one sentinel pattern, and a
guard of sentinel rows lies behind the region.  (a) keep and kept equal the model's and what roman_shared_ids_dev writes, keep
untouched behind each list's kept entries; (b) the slot rows [0, kept) of either side of every affected problem are the pool rows
at off + keep[..], compared as uint64; (c) every other word of the region and the guard still holds the sentinel; (d) the pool
rows are unchanged.

Shapes: tests/_shared_ids.edge_batch (empty sides, 1 x 1, 63 x 64, 64 x 65, 65 x 1, 257 x 300, 1030 x 70 across the 1024-id LDS
tile; the 256-thread form) at F in {5, 8, 130, 131} — odd and even (8 / 16 bytes per lane), and more than one trip of 64 lanes at
both widths (130 / 2 = 65 > 64, 131 > 64) —, small_batch (every map at most 64 rows: the one-wave form) at F in {5, 8}, B = 0, a
call in which no problem is affected and one in which every problem is."""
import numpy as np
import pytest

import _shared_ids as si
from _hipmem import Hip

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x7FF0DEADBEEF0001)              # (a NaN pattern no row holds)
GUARD = 3                                             # sentinel rows behind the region


def distinct_rows(rows, F):
    """(rows, F) uint64: finite doubles (exponent field 0x3FF), every word different."""
    w = np.arange(rows * F, dtype=np.uint64).reshape(rows, F)
    return (np.uint64(0x3FF) << np.uint64(52)) | (w * np.uint64(2654435761) % (np.uint64(1) << np.uint64(52)))


def run_reduce(ctx, hip, ids, off1, n1, off2, n2, F):
    """-> the model's and the device's results of one call, and what roman_shared_ids_dev writes for the same call."""
    B, rows = len(n1), len(ids)
    total = int(n1.sum(dtype=np.int64) + n2.sum(dtype=np.int64))
    pool = distinct_rows(rows, F)
    assert len(np.unique(pool)) == pool.size and np.isfinite(pool.view(np.float64)).all()
    feats = np.concatenate([pool, np.full((total + GUARD, F), SENTINEL, dtype=np.uint64)])
    d_feats, d_ids = hip.upload(feats), hip.upload(ids)
    out = {}
    for name in ("reduce", "mark"):
        d_keep = hip.upload(np.full(max(total, 1), -1, np.int32)); d_kept = hip.upload(np.full((max(B, 1), 2), -7, np.int32))
        if name == "reduce":
            ctx.shared_reduce_dev(B, F, d_feats, rows, d_ids, off1, n1, off2, n2, d_keep, d_kept)
        else:
            ctx.shared_ids_dev(B, d_ids, off1, n1, off2, n2, d_keep, d_kept)
        ctx.sync()
        out[name] = (hip.download(d_keep, (total,), np.int32), hip.download(d_kept, (B, 2), np.int32))
    return pool, hip.download(d_feats, feats.shape, np.uint64), out


def check(pool, feats, out, ids, off1, n1, off2, n2):
    """Assertions (a) - (d) -> (affected problems, problems)."""
    rows, B = pool.shape[0], len(n1)
    want_keep, want_kept = si.mark(ids, off1, n1, off2, n2)
    for name in ("reduce", "mark"):                                            # (a)
        keep, kept = out[name]
        si.compare_written(keep, kept, want_keep, want_kept, n1, n2)
        assert np.array_equal(keep, want_keep), f"{name}: an entry behind a list's kept ones was written"
    assert np.array_equal(feats[:rows], pool), "(d) the pool rows changed"
    expect = np.full_like(feats[rows:], SENTINEL)
    kb, affected = 0, 0
    for b, (k1, k2) in enumerate(si.kept_lists(want_keep, want_kept, n1, n2)):
        if len(k1) != n1[b] or len(k2) != n2[b]:
            affected += 1
            expect[kb:kb + len(k1)] = pool[off1[b] + k1]
            expect[kb + n1[b]:kb + n1[b] + len(k2)] = pool[off2[b] + k2]
        kb += int(n1[b]) + int(n2[b])
    assert np.array_equal(feats[rows:], expect), "(b) / (c): a slot row differs from its pool row, or a word outside the kept rows was written"
    return affected, B


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.free_all()


@pytest.mark.parametrize("F", [5, 8, 130, 131])
def test_edge_batch_256_thread_form(ctx, hip, F):
    ids, off1, n1, off2, n2, names = si.edge_batch()
    assert n1.max() > si.TILE and set(names) >= {"n1 = 0", "n2 = 0", "both empty", "1 x 1 equal", "63 x 64", "64 x 65", "65 x 1", "257 x 300", "1030 x 70"}
    pool, feats, out = run_reduce(ctx, hip, ids, off1, n1, off2, n2, F)
    affected, B = check(pool, feats, out, ids, off1, n1, off2, n2)
    assert 0 < affected < B                                  # both kinds of problem in one call
    hip.free_all()


@pytest.mark.parametrize("F", [5, 8])
def test_small_batch_one_wave_form(ctx, hip, F):
    ids, off1, n1, off2, n2 = si.small_batch()
    assert max(n1.max(), n2.max()) == 64
    pool, feats, out = run_reduce(ctx, hip, ids, off1, n1, off2, n2, F)
    affected, B = check(pool, feats, out, ids, off1, n1, off2, n2)
    assert 0 < affected < B
    hip.free_all()


@pytest.mark.parametrize("form", ["one wave", "256 threads"])
def test_no_problem_affected_and_every_problem_affected(ctx, hip, form):
    m = 40 if form == "one wave" else 100
    rng = np.random.default_rng(5)
    ids = rng.permutation(10 * m)[:6 * m].astype(np.int64) - 1000               # six maps of distinct ids
    off = np.arange(6, dtype=np.int64) * m
    n = np.full(3, m, dtype=np.int32)
    for F in (6, 7):
        pool, feats, out = run_reduce(ctx, hip, ids, off[0::2], n, off[1::2], n, F)
        assert check(pool, feats, out, ids, off[0::2], n, off[1::2], n) == (0, 3)
        assert np.all(feats[pool.shape[0]:] == SENTINEL)                         # the region stays all sentinel
    shared = ids.copy()
    shared[off[1]:off[1] + 1] = shared[off[0]]                                   # one id, all ids, all but one id shared
    shared[off[3]:off[3] + m] = rng.permutation(shared[off[2]:off[2] + m])
    shared[off[5]:off[5] + m - 1] = shared[off[4] + 1:off[4] + m]
    for F in (6, 7):
        pool, feats, out = run_reduce(ctx, hip, shared, off[0::2], n, off[1::2], n, F)
        assert check(pool, feats, out, shared, off[0::2], n, off[1::2], n) == (3, 3)
    hip.free_all()


def test_no_problems(ctx):
    z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    ctx.shared_reduce_dev(0, 5, None, 0, None, z64, z32, z64, z32, None, None)   # B = 0 is legal and enqueues nothing
    ctx.sync()
