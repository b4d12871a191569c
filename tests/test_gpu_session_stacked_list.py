"""roman_session_stacked_sim_list* on the device: the listed pairs' entries BITWISE what
roman_session_stacked_sim_dev writes at the same dense positions over the SAME tables on the SAME device, every other entry and the
guards untouched.  No tolerance anywhere.  The whole-block run of a (d, block list) is made once and shared by all its lists."""
import ctypes

import numpy as np
import pytest

import _frame_desc_oracle as fo
import test_gpu_session_gate_list as tgl
import test_gpu_session_stacked as tss
from _hipmem import Hip
from roman_amd.runtime import session_tables
from test_gpu_grid_gate import FILL, Guarded
from test_session_update_stacked_abi import check_error_codes

pytestmark = pytest.mark.gpu

DIMS = [3, 19, 64]      # the ragged tail only; one full step of 16 and a tail; full steps only
A, B, C, ONE, NO_FRAMES, NO_SUBMAPS = range(6)


def make_session(d):
    """Six robots over one frame table.  A chunk is 32 selected frames (a tile's rows or columns).
      A  70 frames, 5 submaps: the whole map (3 chunks), an empty mask, {a frame opposed to `lean`, a zero-norm frame}, exactly 32
         frames, bits in the second — partial — word only
      B  130 frames, 5 submaps: the whole map (5 chunks), exactly 33 frames (a chunk and one), the six frames that lean one way,
         one frame, exactly 32 frames across a word boundary
      C  33 frames, 3 submaps: the whole map (exactly 33), three identical frames, the last frame alone
      ONE one frame, one submap;  NO_FRAMES three submaps, no frame;  NO_SUBMAPS 70 frames, no submap
    Frames 0..2 of A, B and C are one vector each; `lean` is shared, so A's mask 2 against B's mask 2 is a zero among negative cosines."""
    rng = np.random.default_rng(9700 + d)
    lean = np.abs(rng.normal(0.0, 1.0, d)) + 0.5
    ar = lambda *x: np.array(x, dtype=np.int64)
    pick = lambda Nf, k: np.sort(rng.permutation(Nf)[:k]).astype(np.int64)
    sels = {A: [np.arange(70), ar(), ar(10, 11), np.arange(20, 52), np.arange(64, 70)],
            B: [np.arange(130), pick(130, 33), np.arange(124, 130), ar(77), np.arange(48, 80)],
            C: [np.arange(33), ar(0, 1, 2), ar(32)],
            ONE: [ar(0)], NO_FRAMES: [ar(), ar(), ar()], NO_SUBMAPS: []}
    frames = {A: 70, B: 130, C: 33, ONE: 1, NO_FRAMES: 0, NO_SUBMAPS: 70}
    made = []
    for r in range(6):
        Nf = frames[r]
        desc = rng.normal(0.0, 1.0, (Nf, d))
        if Nf >= 33:
            desc[Nf - 6:] = lean + 0.05 * rng.normal(0.0, 1.0, (6, d))
            desc[:3] = desc[0]
            desc[10] = -lean; desc[11] = 0.0
        made.append((desc, sels[r]))
    assert [len(x) for x in sels[A]] == [70, 0, 2, 32, 6] and [len(x) for x in sels[B]] == [130, 33, 6, 1, 32] and len(sels[C][0]) == 33
    for a in made:
        for b in made:
            if len(a[0]) and len(b[0]):
                fo.clean(fo.borderline_sim(a[0], a[1], b[0], b[1]), f"d={d}")
    masks = [fo.pack_mask(m[1], len(m[0])) for m in made]
    assert masks[A][4][0] == 0 and masks[A][4][1] == (1 << 6) - 1               # nothing in the first word
    frame_n = np.array([len(m[0]) for m in made], dtype=np.int32)
    frame_lo = np.concatenate([[0], np.cumsum(frame_n)[:-1]]).astype(np.int32)
    mask_off = np.concatenate([[0], np.cumsum([m.size for m in masks])[:-1]]).astype(np.int64)
    return dict(made=made, desc=np.concatenate([m[0] for m in made]), masks=masks, mask=np.concatenate([m.reshape(-1) for m in masks]).astype(np.uint64),
                frame_lo=frame_lo, frame_n=frame_n, mask_off=mask_off, counts=[len(m[1]) for m in made], d=d)


ALL = tss.all_pairs(6)
_DENSE = {}


def dense(ctx, d, blocks=ALL, views=None):
    """(session, whole-block similarity, tables) of a case, computed once."""
    key = (d, tuple(blocks), None if views is None else tuple(views))
    if key not in _DENSE:
        hip = Hip()
        try:
            s = make_session(d)
            sim, tabs = tss.run_session(ctx, hip, s, blocks, views=views)
        finally:
            hip.free_all()
        sim.setflags(write=False)
        _DENSE[key] = (s, sim, tabs)
    return _DENSE[key]


def run_list(ctx, hip, s, tabs, lst, shift=0):
    """-> sim (total,) of the list call over a sentinel-filled, guarded buffer; frame table and sim moved off their natural
    position by `shift` doubles."""
    lo, n, mo, sub_off, blk, pair_off = tabs
    lst = np.ascontiguousarray(lst, dtype=np.int32).reshape(-1, 3)
    out = Guarded(hip, int(pair_off[-1]), np.float64, FILL["sim"], shift)
    desc_ptr = hip.upload(np.concatenate([np.zeros(shift), s["desc"].ravel()])) + 8 * shift
    ctx.session_stacked_sim_list_dev(s["d"], len(s["desc"]), desc_ptr, hip.upload(s["mask"]), lo, n, mo, sub_off, blk, pair_off, lst,
                                     hip.upload(lo), hip.upload(n), hip.upload(mo), hip.upload(sub_off), hip.upload(blk), hip.upload(pair_off),
                                     hip.upload(lst) if len(lst) else None, out.ptr)
    ctx.sync()
    return out.get()


def positions(tabs, lst):
    _, _, _, sub_off, blk, pair_off = tabs
    lst = np.asarray(lst, dtype=np.int64).reshape(-1, 3)
    n1 = np.diff(sub_off)[np.asarray(blk).reshape(-1, 4)[lst[:, 0], 1]].astype(np.int64)
    return np.asarray(pair_off)[lst[:, 0]] + lst[:, 1] * n1 + lst[:, 2]


def full_list(tabs):
    _, _, _, sub_off, blk, _ = tabs
    c = np.diff(sub_off)
    return np.array([(b, i, j) for b, (r0, r1, _, _) in enumerate(np.asarray(blk).reshape(-1, 4).tolist()) for i in range(c[r0]) for j in range(c[r1])],
                    dtype=np.int32).reshape(-1, 3)


def lists_of(tabs):
    full = full_list(tabs)
    cut = np.searchsorted(full[:, 0], np.arange(len(tabs[4]) + 1))
    ends = np.array(sorted({int(k) for b in range(len(tabs[4])) if cut[b + 1] > cut[b] for k in (cut[b], cut[b + 1] - 1)}), dtype=np.int64)
    self_b = [b for b, x in enumerate(np.asarray(tabs[4]).reshape(-1, 4).tolist()) if x[0] == x[1] and cut[b + 1] > cut[b]]
    one = cut[1] + 3 * 5 + 1                                 # block (A, B), pair (3, 1): exactly 32 frames against 33 — one row chunk, two column chunks
    return dict(empty=full[:0], one_pair=full[one:one + 1], every_pair=full, first_and_last_of_each_block=full[ends],
                a_self_block=full[cut[self_b[1]]:cut[self_b[1] + 1]], every_third=full[::3])


def check(got, want, tabs, lst, tag):
    at = positions(tabs, lst)
    rest = np.ones(len(want), dtype=bool); rest[at] = False
    assert got[at].tobytes() == want[at].tobytes(), (tag, got[at], want[at])
    assert (got[rest] == FILL["sim"]).all(), (tag, "an entry that is not listed was written")


@pytest.mark.parametrize("d", DIMS)
def test_listed_pairs_equal_the_whole_block_call_bitwise(ctx, d):
    """Every list over all r <= s of the six robots; shifted buffers and a second run give the same bits; the host twin equals
    the device call and returns the entries that are not listed as they were given."""
    s, want, tabs = dense(ctx, d)
    pair_off, blocks = tabs[5], ALL
    at = lambda r0, r1, i, j: int(pair_off[blocks.index((r0, r1, r0 == r1))]) + i * s["counts"][r1] + j
    assert want[at(A, B, 2, 2)] == 0.0                                           # the zero-norm frame among negative cosines
    assert np.isneginf(want[at(A, B, 1, 0)]) and np.isneginf(want[at(A, NO_FRAMES, 0, 0)]) and np.isneginf(want[at(NO_FRAMES, NO_FRAMES, 1, 1)])
    hip = Hip()
    try:
        for name, lst in lists_of(tabs).items():
            got = run_list(ctx, hip, s, tabs, lst)
            check(got, want, tabs, lst, (d, name))
            if name in ("every_pair", "every_third"):
                again = run_list(ctx, hip, s, tabs, lst, shift=1)
                assert again.tobytes() == got.tobytes(), (d, name, "a shifted run differs")
            if name == "every_pair":
                assert got.tobytes() == want.tobytes()
            if name == "every_third":                        # the host twin
                given = np.full(len(want), FILL["sim"]); given[::5] = 7.5
                host = ctx.session_stacked_sim_list(s["desc"], s["mask"], *tabs, lst, sim=given.copy())
                listed = np.zeros(len(want), dtype=bool); listed[positions(tabs, lst)] = True
                assert host[listed].tobytes() == want[listed].tobytes() and host[~listed].tobytes() == given[~listed].tobytes()
                fresh = ctx.session_stacked_sim_list(s["desc"], s["mask"], *tabs, lst)
                assert fresh[listed].tobytes() == want[listed].tobytes() and np.isnan(fresh[~listed]).all()
    finally:
        hip.free_all()


def test_a_pair_does_not_depend_on_the_other_pairs_listed(ctx):
    """Every pair listed alone in a call of its own (d = 19, the blocks of A, B and C) gives the bits it has in the full list."""
    blocks = [(A, B, False), (B, C, False), (C, A, False)]
    s, want, tabs = dense(ctx, 19, blocks)
    hip = Hip()
    try:
        full = full_list(tabs)
        for k in range(0, len(full), 4):
            got = run_list(ctx, hip, s, tabs, full[k:k + 1])
            check(got, want, tabs, full[k:k + 1], ("alone", full[k].tolist()))
    finally:
        hip.free_all()


def test_two_views_of_one_robot_read_the_same_frames_and_words(ctx):
    """Views 0 and 1 are robot A (one frame range, one set of mask words), view 2 is robot B."""
    views, blocks = [A, A, B], [(0, 2, False), (1, 2, False), (0, 1, False), (2, 1, False)]
    s, want, tabs = dense(ctx, 19, blocks, views)
    assert tabs[0][0] == tabs[0][1] and tabs[2][0] == tabs[2][1]
    hip = Hip()
    try:
        for name, lst in (("every_pair", full_list(tabs)), ("every_third", full_list(tabs)[::3])):
            check(run_list(ctx, hip, s, tabs, lst), want, tabs, lst, ("aliased views", name))
    finally:
        hip.free_all()


def test_the_list_gate_reads_this_buffer_as_it_reads_the_whole_block_calls(ctx):
    """roman_session_gate_list_dev(sim_in = the list call's buffer, the sentinel everywhere else) equals the same call over the
    whole-block buffer, every output bitwise."""
    counts = (5, 5, 3)
    blocks = tss.all_pairs(3)
    s, want, tabs = dense(ctx, 19, blocks, [A, B, C])
    assert tuple(np.diff(tabs[3]).tolist()) == counts and np.array_equal(tabs[5], session_tables(counts, blocks)[2])
    hip = Hip()
    try:
        lst = full_list(tabs)[::3]
        sparse = run_list(ctx, hip, s, tabs, lst)
        assert (sparse == FILL["sim"]).sum() == len(want) - len(lst)
        gate = dict(tgl.GATE, desc_thresh=0.8)
        outs = [tgl.Session(ctx, hip, 9800, counts, 0, blocks, gate=gate, mode="sim", sim_in=np.array(buf)).run_list(lst) for buf in (want, sparse)]
        for k in outs[0]:
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
        assert outs[0]["sim"].tobytes() == want[positions(tabs, lst)].tobytes()
        listed = want[positions(tabs, lst)]
        assert (listed < gate["desc_thresh"]).any() and (listed >= gate["desc_thresh"]).any(), "the similarity decides nothing"
    finally:
        hip.free_all()


def test_without_a_live_block_desc_and_mask_may_be_null(ctx):
    """Blocks between robots with frames and the robot with submaps and no frame: Nf > 0, L > 0, and no pair reads a frame.  desc
    and mask are NULL; every listed pair is -inf, every other entry holds the sentinel — device call and host twin."""
    blocks = [(A, NO_FRAMES, False), (NO_FRAMES, B, False)]
    s = make_session(19)
    sub_off, blk, pair_off, _ = session_tables(s["counts"], blocks)
    tabs = (s["frame_lo"], s["frame_n"], s["mask_off"], sub_off, blk, pair_off)
    lst = np.ascontiguousarray(full_list(tabs)[::2])              # (handed to the C entry as it is)
    assert len(s["desc"]) > 0 and len(lst) > 0
    hip = Hip()
    try:
        out = Guarded(hip, int(pair_off[-1]), np.float64, FILL["sim"])
        ctx.session_stacked_sim_list_dev(s["d"], len(s["desc"]), None, None, *tabs, lst, *[hip.upload(t) for t in tabs], hip.upload(lst), out.ptr)
        ctx.sync()
        got = out.get()
        listed = np.zeros(len(got), dtype=bool); listed[positions(tabs, lst)] = True
        assert np.isneginf(got[listed]).all() and (got[~listed] == FILL["sim"]).all()
        lib, p = ctx._lib, lambda x: ctypes.c_void_p(x.ctypes.data)
        host = np.full(len(got), FILL["sim"])
        rc = lib.roman_session_stacked_sim_list(ctx._h, s["d"], len(s["desc"]), None, None, len(s["mask"]), len(s["counts"]), p(tabs[0]), p(tabs[1]), p(tabs[2]),
                                                p(sub_off), len(blk), p(blk), p(pair_off), len(lst), p(lst), p(host))
        assert rc == 0 and host.tobytes() == got.tobytes()
    finally:
        hip.free_all()


def test_error_codes(ctx):
    check_error_codes(ctx._lib, ctx._h)
    ctx.sync()
    hip = Hip()
    try:                                                     # L == 0 on a live context: ROMAN_OK, nothing written
        s, want, tabs = dense(ctx, 3)
        got = run_list(ctx, hip, s, tabs, np.zeros((0, 3), np.int32))
        assert (got == FILL["sim"]).all()
    finally:
        hip.free_all()
