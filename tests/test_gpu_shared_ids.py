"""The shared-segment removal of self loop closures on the GPU: roman_shared_ids_dev against the NumPy model
(tests/_shared_ids.py), roman_align_lc_batch_ids against today's path — roman_align_lc_batch on the 2 B pool the host builds
from the reduced lists — bit for bit, unchunked and chunked, the refusal of explicit association lists, and a demo-scale grid of
one robot against itself through both whole functions."""
import copy

import numpy as np
import pytest

import _shared_ids as si
from _hipmem import Hip
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams, batch as rb
from roman_amd.align import submap_align as sa
from roman_amd.runtime import Context
from test_gpu_submap_align_grid import random_lc
from test_submap_align_grid_cpu import compare_with_pair_loop

pytestmark = pytest.mark.gpu


def run_mark(ctx, hip, ids, off1, n1, off2, n2):
    total = int(n1.sum() + n2.sum()); B = len(n1)
    d_ids = hip.upload(ids)
    d_keep = hip.upload(np.full(max(total, 1), -1, np.int32)); d_kept = hip.upload(np.full((max(B, 1), 2), -7, np.int32))
    ctx.shared_ids_dev(B, d_ids, off1, n1, off2, n2, d_keep, d_kept)
    ctx.sync()
    return hip.download(d_keep, (total,), np.int32), hip.download(d_kept, (B, 2), np.int32)


def test_shared_ids_dev_matches_the_model(ctx):
    """One call over the edge batch (empty sides, 1 x 1, sizes around one wave / one workgroup / one LDS tile of 1024 ids — the
    pair (1030, 70) crosses the tile on one side and takes five chunks of 256 own objects on the other —, all / none shared, ids
    that differ in their high words only, negative ids, repetitions inside a map, the same slice on both sides, slices shared
    between problems); one call whose maps all fit a wave (the kernel's one-wave-per-problem form); B = 0."""
    hip = Hip()
    try:
        ids, off1, n1, off2, n2, names = si.edge_batch()
        assert n1.max() > si.TILE and set(names) >= {"1030 x 70", "63 x 64", "64 x 65", "65 x 1", "257 x 300"}
        keep, kept = run_mark(ctx, hip, ids, off1, n1, off2, n2)
        want_keep, want_kept = si.mark(ids, off1, n1, off2, n2)
        si.compare_written(keep, kept, want_keep, want_kept, n1, n2)
        assert np.array_equal(keep, want_keep)               # nothing written behind a list's kept entries (the -1 fill survives)
        ids, off1, n1, off2, n2 = si.small_batch()
        assert max(n1.max(), n2.max()) == 64
        keep, kept = run_mark(ctx, hip, ids, off1, n1, off2, n2)
        want_keep, want_kept = si.mark(ids, off1, n1, off2, n2)
        si.compare_written(keep, kept, want_keep, want_kept, n1, n2)
        assert np.array_equal(keep, want_keep)
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        ctx.shared_ids_dev(0, None, z64, z32, z64, z32, None, None)            # B = 0 is legal
        ctx.sync()
    finally:
        hip.free_all()


@pytest.fixture(scope="module")
def planted():
    """48 pairs of maps of 20-40 objects, d = 16, method 'roman', over one pool; shared ids planted in about half of them (between
    one and all objects); pair 5 is left with 2 objects per side, pair 7 is emptied on side 1 only (its ids all occur in map 2,
    some of them repeated).  -> registration, batch with ids, tail inputs, the model's lists and today's 2 B batch."""
    reg = SubmapAlignParams(method="roman", semantics_dim=16).get_object_registration()
    rng = np.random.default_rng(77)
    sizes = [(int(rng.integers(20, 41)), int(rng.integers(20, 41))) for _ in range(48)]
    sizes[5] = (30, 30); sizes[7] = (25, 30)
    pairs = [synth.make_pair(a, c, 16, 5200 + k) for k, (a, c) in enumerate(sizes)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    ids = (np.arange(batch.feats.shape[0], dtype=np.int64) + 1) * 1000003 - (1 << 40)      # distinct, some negative, beyond 32 bits
    for b, (a, c) in enumerate(sizes):
        o1, o2 = int(batch.off1[b]), int(batch.off2[b])
        if b == 5:
            share = a - 2
        elif b == 7:
            ids[o1:o1 + a] = ids[o2 + rng.integers(0, 25, a)]                              # every id of map 1 is one of 25 ids of map 2
            continue
        elif b % 2:
            share = int(rng.integers(1, min(a, c) + 1)) if b % 6 != 1 else min(a, c)
        else:
            continue
        ids[o2 + rng.permutation(c)[:share]] = ids[o1 + rng.permutation(a)[:share]]
    lc = random_lc(48, np.random.default_rng(8), thresh=5)
    batch.ids = ids
    f2, o1, m1, o2, m2, keep, kept = si.reduce_on_host(batch.feats, ids, batch.off1, batch.n1, batch.off2, batch.n2)
    assert tuple(kept[5]) == (2, 2) and kept[7, 0] == 0 and kept[7, 1] > 0
    affected = (kept[:, 0] != batch.n1) | (kept[:, 1] != batch.n2)
    assert 20 <= affected.sum() <= 28 and (kept[affected].min(axis=1) == 0).sum() >= 2
    return reg, batch, lc, keep, kept, rb.AlignmentBatch(f2, o1, m1, o2, m2)


def assert_same_result(got, want):
    assert np.array_equal(got.status, want.status)
    assert len(got.assoc) == len(want.assoc)
    for b in range(len(want.assoc)):
        assert np.array_equal(got.assoc[b], want.assoc[b]), b
    assert np.array_equal(got.T, want.T, equal_nan=True)
    assert got.records.tobytes() == want.records.tobytes()
    assert np.array_equal(got.accepted, want.accepted)


@pytest.fixture(scope="module")
def unchunked(planted):
    reg, batch, lc, keep, kept, reduced = planted
    c = Context(0)
    try:
        reg.set_context(c)
        want = rb.run_lc_batch(reg, reduced, lc)             # today's path: the reduced lists packed into a 2 B pool on the host
        got = c.align_lc_batch_ids(reg._abi_params(), batch.feats, batch.ids, batch.off1, batch.n1, batch.off2, batch.n2, lc, kmax=reduced.kmax())
    finally:
        reg.set_context(None); c.close()
    return want, got


def test_align_lc_batch_ids_equals_the_per_pair_path_bit_for_bit(planted, unchunked):
    reg, batch, lc, keep, kept, reduced = planted
    want, got = unchunked
    assert_same_result(got, want)                            # the same kernels on bit-copied rows: no tolerance
    assert np.array_equal(got.n1_kept, kept[:, 0]) and np.array_equal(got.n2_kept, kept[:, 1])
    si.compare_written(got.keep, np.stack([got.n1_kept, got.n2_kept], axis=1), keep, kept, batch.n1, batch.n2)
    assert got.status[7] & _abi.ROMAN_ST_EMPTY_MAP and got.status[5] & _abi.ROMAN_ST_INSUFFICIENT
    assert len(got.accepted) > 5 and not (got.status & (_abi.ROMAN_ST_WORKSPACE | _abi.ROMAN_ST_INTERNAL)).any()


def test_chunked_call_with_calls_in_flight_equals_the_unchunked_one(planted, unchunked):
    reg, batch, lc, keep, kept, reduced = planted
    c = Context(0)
    try:
        c.set_host_batching(16, 3)                           # 48 problems: three calls of 16, all in flight behind the first
        got = c.align_lc_batch_ids(reg._abi_params(), batch.feats, batch.ids, batch.off1, batch.n1, batch.off2, batch.n2, lc, kmax=reduced.kmax())
    finally:
        c.close()
    assert_same_result(got, unchunked[1])
    assert np.array_equal(got.n1_kept, kept[:, 0]) and np.array_equal(got.n2_kept, kept[:, 1])


def test_explicit_lists_with_ids_are_refused(ctx, planted):
    reg, batch, lc, keep, kept, reduced = planted
    from roman_amd.clipperpy.utils import create_all_to_all
    lists = [create_all_to_all(int(a), int(c)) for a, c in zip(batch.n1, batch.n2)]
    assoc_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    with pytest.raises(_abi.RomanHipError, match=r"\(-1\).*assoc"):                          # ROMAN_E_INVALID, with a message
        ctx.align_lc_batch_ids(reg._abi_params(), batch.feats, batch.ids, batch.off1, batch.n1, batch.off2, batch.n2, lc,
                               assoc=np.concatenate(lists), assoc_off=assoc_off)
    sub = slice(4, 9)                                        # ... and the context goes on working
    got = ctx.align_lc_batch_ids(reg._abi_params(), batch.feats, batch.ids, batch.off1[sub], batch.n1[sub], batch.off2[sub], batch.n2[sub],
                                 LcRows(lc, sub))
    assert np.array_equal(got.n1_kept, kept[sub, 0]) and np.array_equal(got.n2_kept, kept[sub, 1])


def LcRows(lc, rows):
    """The tail inputs of a run of problems."""
    out = copy.copy(lc)
    out.T_ref, out.enable, out.iL, out.iR = lc.T_ref[rows], lc.enable[rows], lc.iL[rows], lc.iR[rows]
    return out


def test_demo_scale_self_grid(ctx, tmp_path):
    """One robot against itself: 12 submaps of 20-40 objects with 768-d descriptors, neighbours sharing a third of their segments
    (the id ranges of consecutive submaps overlap), every submap sharing all of them with itself; a time gate that stops accepted
    pairs.  submap_align_grid (the removal on the device, every submap uploaded once) against submap_align (the removal per pair
    on the host)."""
    params = SubmapAlignParams(method="roman", semantics_dim=768, single_robot_lc=True, single_robot_lc_time_thresh=50.0, submap_radius=1e3)
    reg = params.get_object_registration(); reg.set_context(ctx)
    rng = np.random.default_rng(4)
    objs, poses = synth.make_submap_grid(12, n=40, d=768, seed0=8300, overlap=0.6)
    objs = [[o[q] for q in sorted(rng.choice(40, size=int(rng.integers(20, 41)), replace=False))] for o in objs]
    start = 0
    for segs in objs:
        for q, s in enumerate(segs):
            s.id = start + q
        start += len(segs) - len(segs) // 3
    robot = [sa.Submap(id=k, time=20.0 * k, segments=objs[k],
                       pose_flu=poses[k] @ synth.yaw_transform(0.0, [0, 0, 0], roll=rng.normal(0, 0.02), pitch=rng.normal(0, 0.02))) for k in range(12)]
    submaps = [robot, copy.deepcopy(robot)]
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    old, new, edges = compare_with_pair_loop(params, io, submaps, None, tmp_path, old_compute=None, new_compute=None, registration=reg)
    dt = np.abs(np.array([[a.time - b.time for b in robot] for a in robot]))
    enough = old.clipper_num_associations >= 4
    assert (enough & (dt < 50.0)).any() and len(edges) == int(np.count_nonzero(enough & ~(dt < 50.0))) > 0
    assert np.all(np.diag(old.clipper_num_associations) == 0)                  # a submap against itself: nothing is left
    shared = np.array([[len({s.id for s in a.segments} & {s.id for s in b.segments}) for b in robot] for a in robot])
    assert np.all(np.diag(shared, 1) > 0) and np.all(np.triu(shared, 2) == 0)
