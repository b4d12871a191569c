"""roman_session_stacked_sim* and roman_session_gate_sim* on the device.

The similarity of every block BITWISE against roman_stacked_sim_dev called on the block's two sides on the SAME device, and against
the NumPy oracle with the rule of tests/test_gpu_frame_desc.py (`close`, inputs without a borderline flag); the gate over a given
similarity per block BITWISE against roman_grid_gate_sim_dev on that block's slice."""
import numpy as np
import pytest

import _frame_desc_oracle as fo
import _session_stacked as st
import test_gpu_frame_desc as tg
import test_gpu_session_gate as tsg
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import grid_gate_params, session_tables
from test_gpu_grid_gate import DTYPE, FILL, Guarded
from test_session_stacked_abi import check_error_codes

pytestmark = pytest.mark.gpu

# (frames, submaps) per robot: 70 and 130 frames end in a partial mask word, a band of 32 rows cuts inside a word at 32 and at 96;
# a robot of one frame, one without frames, one without submaps
ROBOTS = [(70, 5), (130, 3), (33, 5), (1, 1), (0, 3), (70, 0)]


def all_pairs(R):
    return [(r, s, r == s) for r in range(R) for s in range(r, R)]


def make_robot(rng, Nf, S, d):
    """-> (desc (Nf, d), sel: S ascending index arrays).  With three submaps or more: one whole-map mask, one empty mask, and one
    {zero-norm frame, the negative of a direction the robot's last frames lean towards}; frames 0 .. 2 are one vector."""
    desc = rng.normal(0.0, 1.0, (Nf, d))
    sel = [np.sort(rng.permutation(Nf)[:int(rng.integers(1, max(2, Nf // 2 + 1)))]).astype(np.int64) if Nf else np.zeros(0, np.int64) for _ in range(S)]
    if Nf >= 33:
        lean = np.abs(rng.normal(0.0, 1.0, d)) + 0.5
        desc[Nf - 6:] = lean + 0.05 * rng.normal(0.0, 1.0, (6, d))
        desc[:3] = desc[0]
        desc[10] = -lean; desc[11] = 0.0
        if S >= 3:
            sel[0] = np.arange(Nf); sel[1] = np.zeros(0, np.int64); sel[2] = np.array([10, 11])
            if S >= 5:
                sel[3] = np.arange(Nf - 6, Nf); sel[4] = np.array([1, Nf - 1])          # (Nf - 1: the last bit of a partial word)
    return desc, sel


def make_session(seed, d, robots=ROBOTS):
    rng = np.random.default_rng(seed)
    made = [make_robot(rng, Nf, S, d) for Nf, S in robots]
    for a in made:
        for b in made:
            if len(a[0]) and len(b[0]):
                fo.clean(fo.borderline_sim(a[0], a[1], b[0], b[1]), f"session seed {seed} d={d}")
    desc = np.concatenate([m[0] for m in made])
    masks = [fo.pack_mask(m[1], len(m[0])) for m in made]
    frame_n = np.array([len(m[0]) for m in made], dtype=np.int32)
    frame_lo = np.concatenate([[0], np.cumsum(frame_n)[:-1]]).astype(np.int32)
    words = [m.size for m in masks]
    mask_off = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
    return dict(made=made, desc=desc, masks=masks, mask=np.concatenate([m.reshape(-1) for m in masks]).astype(np.uint64), frame_lo=frame_lo,
                frame_n=frame_n, mask_off=mask_off, counts=[len(m[1]) for m in made], d=d)


def run_session(ctx, hip, s, blocks, shift=0, views=None):
    """-> (sim (total,), the tables).  `views`: robot index per table entry (default: every robot once); `shift`: doubles the frame
    table and sim are moved off their natural position (one double leaves a 16-byte boundary; the row pitch is d * 8 bytes)."""
    views = list(range(len(s["counts"]))) if views is None else views
    sub_off, blk, pair_off, _ = session_tables([s["counts"][r] for r in views], blocks)
    lo, n, mo = s["frame_lo"][views].copy(), s["frame_n"][views].copy(), s["mask_off"][views].copy()
    total = int(pair_off[-1])
    out = Guarded(hip, total, np.float64, FILL["sim"], shift)
    desc_ptr = hip.upload(np.concatenate([np.zeros(shift), s["desc"].ravel()])) + 8 * shift
    ctx.session_stacked_sim_dev(s["d"], len(s["desc"]), desc_ptr, hip.upload(s["mask"]), lo, n, mo, sub_off, blk, pair_off,
                                hip.upload(lo), hip.upload(n), hip.upload(mo), hip.upload(sub_off), hip.upload(blk), hip.upload(pair_off), out.ptr)
    ctx.sync()
    return out.get(), (lo, n, mo, sub_off, blk, pair_off)


def block_reference(ctx, hip, s, r0, r1):
    """roman_stacked_sim_dev on the two sides of a block, each side in buffers of its own."""
    (d0, _), (d1, _) = s["made"][r0], s["made"][r1]
    S0, S1 = s["counts"][r0], s["counts"][r1]
    out = Guarded(hip, S0 * S1, np.float64, FILL["sim"])
    ctx.stacked_sim_dev(s["d"], len(d0), hip.upload(d0), S0, hip.upload(s["masks"][r0]), len(d1), hip.upload(d1), S1, hip.upload(s["masks"][r1]), out.ptr)
    ctx.sync()
    return out.get()


def check_blocks(ctx, hip, s, got, blocks, views=None, tag=""):
    views = list(range(len(s["counts"]))) if views is None else views
    at = 0
    for v0, v1, _ in blocks:
        r0, r1 = views[v0], views[v1]
        n = s["counts"][r0] * s["counts"][r1]
        if n:
            want = block_reference(ctx, hip, s, r0, r1)
            assert got[at:at + n].tobytes() == want.tobytes(), (tag, (v0, v1), got[at:at + n], want)
            oracle = fo.stacked_sim_oracle(s["made"][r0][0], s["made"][r0][1], s["made"][r1][0], s["made"][r1][1])
            assert tg.close(got[at:at + n].reshape(oracle.shape), oracle), (tag, (v0, v1))
        at += n
    assert at == len(got)


@pytest.mark.parametrize("d", [3, 19, 64])
def test_every_block_equals_stacked_sim_dev_bitwise_at_every_band_height(ctx, d):
    """All r <= s over ROBOTS.  Band 32: a block of 130 frames takes five rounds, one of 33 two, one of 1 one — the blocks leave the
    rounds at different times; the default band: one round.  Both give the bits of roman_stacked_sim_dev, and of each other."""
    s = make_session(9100 + d, d)
    blocks = all_pairs(len(ROBOTS))
    hip = Hip()
    try:
        whole, tabs = run_session(ctx, hip, s, blocks)
        again, _ = run_session(ctx, hip, s, blocks, shift=1)
        ctx.set_stacked_band(_abi.STACKED_BAND_MIN)
        banded, _ = run_session(ctx, hip, s, blocks, shift=1)
        ctx.set_stacked_band(0)
        assert whole.tobytes() == again.tobytes() and whole.tobytes() == banded.tobytes()
        check_blocks(ctx, hip, s, whole, blocks, tag=f"d={d}")
        want, per = st.session_stacked_oracle(s["desc"], s["mask"], *tabs[:5])
        assert np.array_equal(np.isneginf(whole), np.isneginf(want))
        b07 = per[blocks.index((0, 2, False))]
        assert b07[2, 3] == 0.0 and whole[int(tabs[5][blocks.index((0, 2, False))]) + 2 * 5 + 3] == 0.0       # the zero-norm frame among negative cosines
        assert np.isneginf(per[blocks.index((0, 4, False))]).all() and np.isneginf(per[0][1]).all()           # a view without frames; an empty mask
        host = ctx.session_stacked_sim(s["desc"], s["mask"], *tabs)
        assert host.tobytes() == whole.tobytes()
    finally:
        ctx.set_stacked_band(0)
        hip.free_all()


LISTS = dict(off_diagonal=[(r, s, False) for r in range(len(ROBOTS)) for s in range(len(ROBOTS)) if r != s][::3], one_self_block=[(1, 1, True)], empty=[])


@pytest.mark.parametrize("name", sorted(LISTS))
def test_block_lists(ctx, name):
    s = make_session(9200, 19)
    blocks = LISTS[name]
    hip = Hip()
    try:
        ctx.set_stacked_band(_abi.STACKED_BAND_MIN)
        got, _ = run_session(ctx, hip, s, blocks)
        check_blocks(ctx, hip, s, got, blocks, tag=name)
        assert len(got) == sum(s["counts"][a] * s["counts"][b] for a, b, _ in blocks)
    finally:
        ctx.set_stacked_band(0)
        hip.free_all()


def test_two_views_of_one_robot_read_the_same_frames_and_words(ctx):
    """Views 0 and 1 are robot 0 (the same frame range, the same mask words), view 2 is robot 1: (0, 2) and (1, 2) are one matrix, and
    (0, 1) is robot 0 against itself."""
    s = make_session(9300, 19)
    views, blocks = [0, 0, 1], [(0, 2, False), (1, 2, False), (0, 1, False), (2, 1, False)]
    hip = Hip()
    try:
        ctx.set_stacked_band(_abi.STACKED_BAND_MIN)
        got, tabs = run_session(ctx, hip, s, blocks, views=views)
        assert tabs[0][0] == tabs[0][1] and tabs[2][0] == tabs[2][1]
        check_blocks(ctx, hip, s, got, blocks, views=views, tag="aliased views")
        n = s["counts"][0] * s["counts"][1]
        assert got[:n].tobytes() == got[n:2 * n].tobytes()
    finally:
        ctx.set_stacked_band(0)
        hip.free_all()


def test_error_codes(ctx):
    check_error_codes(ctx._lib, ctx._h)
    ctx.sync()


# ---------------------------------------------------------------------------------------------
# the session gate over a given similarity
# ---------------------------------------------------------------------------------------------
OUT = ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable")
GATE = dict(radius=12.0, skip_distance=25.0, desc_thresh=0.6, lc_time_thresh=60.0)


def given_similarity(rng, total, thresh, kind):
    """Entries on both sides of the threshold, and — wherever the list is long enough — exactly at it, one step below, one step
    above, and -inf.  The gate is sim < thresh: equality passes."""
    sim = rng.uniform(0.0, 1.0, total) if kind == "mixed" else np.full(total, {"all": 1.0, "none": -np.inf, "one": 0.0}[kind])
    if kind == "mixed":
        plant = [thresh, np.nextafter(thresh, -np.inf), np.nextafter(thresh, np.inf), -np.inf]
        sim[:len(plant)] = plant[:total]
    if kind == "one":
        sim[total - 1] = thresh
    return sim


def run_gate_sim(ctx, hip, arr, counts, blocks, has_gt, gate, sim_in, shift=0):
    sub_off, blk, pair_off, tile_off = session_tables(counts, blocks)
    total, nb = int(pair_off[-1]), len(blocks)
    up = lambda x: None if x is None or x.size == 0 else hip.upload(np.concatenate([np.zeros(shift), np.asarray(x, dtype=np.float64).ravel()])) + 8 * shift
    out = {k: Guarded(hip, tsg.WIDTH[k] * total, DTYPE[k], FILL[k], shift) for k in OUT}
    out["todo_off"] = Guarded(hip, nb + 1, np.int32, -11, shift)
    given = Guarded(hip, total, np.float64, 0.0, shift)
    assert hip.lib.hipMemcpy(given.ptr, np.ascontiguousarray(sim_in).ctypes.data, 8 * total, 1) == 0 or total == 0
    P = grid_gate_params(desc_dim=0, single_robot_lc=False, **gate)
    ctx.session_gate_dev(P, sub_off, blk, pair_off, tile_off, hip.upload(sub_off), hip.upload(blk), hip.upload(pair_off), hip.upload(tile_off),
                         up(arr["pos"]), up(arr["T_w"]), *[out[k].ptr for k in OUT], out["todo_off"].ptr, time_ptr=up(arr["time"]),
                         pos_gt_ptr=up(arr["pos_gt"]), has_gt_ptr=hip.upload(np.asarray(has_gt, dtype=np.int32)), sim_in_ptr=given.ptr)
    ctx.sync()
    got = {k: v.get() for k, v in out.items()}
    assert (got["sim"] == FILL["sim"]).all(), "sim was written"
    assert np.array_equal(hip.download(given.ptr, (total,), np.float64), sim_in, equal_nan=True), "sim_in was written"
    for k in ("T_ij", "T_ref"):
        got[k] = got[k].reshape(total, 4, 4)
    got["pairs"] = got["pairs"].reshape(total, 2)
    return got, (sub_off, blk, pair_off, tile_off)


def check_against_grid_gate_sim(ctx, hip, got, tabs, sides, counts, blocks, has_gt, gate, sim_in, tag=""):
    sub_off, _, pair_off, _ = tabs
    want_off = [0]
    for b, (r0, r1, lc) in enumerate(blocks):
        n0, n1 = counts[r0], counts[r1]
        lo, hi = int(pair_off[b]), int(pair_off[b + 1])
        if n0 == 0 or n1 == 0:
            want_off.append(want_off[-1]); continue
        gt = bool(has_gt[r0] and has_gt[r1])
        a, bb = sides[r0], sides[r1]
        B = n0 * n1
        up = lambda x: hip.upload(np.asarray(x, dtype=np.float64))
        one = {k: Guarded(hip, tsg.WIDTH[k] * B, DTYPE[k], FILL[k]) for k in OUT if k != "sim"}
        n_todo = Guarded(hip, 1, np.int32, -11)
        P = grid_gate_params(desc_dim=0, single_robot_lc=bool(lc), **gate)
        ctx.grid_gate_sim_dev(P, n0, n1, up(a["pos"]), up(a["T_w"]), up(bb["pos"]), up(bb["T_w"]), one["dist"].ptr, one["flags"].ptr, one["yaw_deg"].ptr,
                              up(sim_in[lo:hi]), one["T_ij"].ptr, one["pairs"].ptr, one["T_ref"].ptr, one["enable"].ptr, n_todo.ptr,
                              time0_ptr=up(a["time"]), time1_ptr=up(bb["time"]), pos_gt0_ptr=up(a["pos_gt"]) if gt else None,
                              pos_gt1_ptr=up(bb["pos_gt"]) if gt else None)
        ctx.sync()
        w = {k: v.get() for k, v in one.items()}
        n = int(n_todo.get()[0])
        for k in ("dist", "flags", "yaw_deg", "T_ij"):
            assert got[k][lo:hi].tobytes() == w[k].tobytes(), (tag, blocks[b], k)
        s0, s1 = want_off[-1], want_off[-1] + n
        assert np.array_equal(got["pairs"][s0:s1], w["pairs"].reshape(B, 2)[:n] + np.array([sub_off[r0], sub_off[r1]], dtype=np.int32)), (tag, blocks[b])
        assert got["T_ref"][s0:s1].tobytes() == w["T_ref"].reshape(B, 4, 4)[:n].tobytes(), (tag, blocks[b], "T_ref")
        assert np.array_equal(got["enable"][s0:s1], w["enable"][:n]), (tag, blocks[b], "enable")
        want_off.append(s1)
    assert got["todo_off"].tolist() == want_off, (tag, got["todo_off"].tolist(), want_off)
    n = want_off[-1]
    assert (got["pairs"][n:] == FILL["pairs"]).all() and (got["T_ref"][n:] == FILL["T_ref"]).all() and (got["enable"][n:] == FILL["enable"]).all()
    return n


@pytest.mark.parametrize("counts", [(1,), (3, 0, 5), (17, 64, 5)], ids=["1", "3-0-5", "17-64-5"])
def test_gate_over_a_given_similarity_equals_grid_gate_sim_dev_bitwise(ctx, counts):
    R = len(counts)
    has_gt = [1] + [0] * (R - 1) if R > 1 else [1]
    blocks = tsg.all_pairs(R)
    sides, arr, g = tsg.make_session(9400 + R + counts[0], counts, 0, has_gt, blocks, GATE)
    total = int(session_tables(counts, blocks)[2][-1])
    sim_in = given_similarity(np.random.default_rng(9401), total, GATE["desc_thresh"], "mixed")
    hip = Hip()
    try:
        g = dict(g, desc_thresh=GATE["desc_thresh"])          # (make_session clears it without descriptors: here it gates sim_in)
        got, tabs = run_gate_sim(ctx, hip, arr, counts, blocks, has_gt, g, sim_in, shift=len(counts) % 2)
        n = check_against_grid_gate_sim(ctx, hip, got, tabs, sides, counts, blocks, has_gt, g, sim_in, tag=str(counts))
        skip = (got["flags"] & _abi.ROMAN_GRID_SKIP) != 0
        gated = (got["flags"] & _abi.ROMAN_GRID_GATED) != 0
        assert np.array_equal(gated, ~skip & (sim_in < g["desc_thresh"])) and n == int((~skip & ~gated).sum())
        if total >= 4 and not skip[:4].any():                 # at, just below, just above the threshold, -inf
            assert gated[:4].tolist() == [False, True, False, True]
        again, _ = run_gate_sim(ctx, hip, arr, counts, blocks, has_gt, g, sim_in)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k
        if len(counts) == 3:                                  # the host-pointer twin
            given = dict(pairs=np.full((total, 2), FILL["pairs"], np.int32), T_ref=np.full((total, 4, 4), FILL["T_ref"]), enable=np.full(total, FILL["enable"], np.int32))
            h = ctx.session_gate(grid_gate_params(desc_dim=0, **g), *tabs, arr["pos"], arr["T_w"], time=arr["time"], pos_gt=arr["pos_gt"], has_gt=has_gt,
                                 sim_in=sim_in, **given)
            for k in ("dist", "flags", "yaw_deg", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
                assert np.asarray(getattr(h, k)).tobytes() == got[k].tobytes(), k
            assert np.array_equal(h.sim, sim_in, equal_nan=True)
    finally:
        hip.free_all()


@pytest.mark.parametrize("kind", ["all", "none", "one"])
def test_gate_all_none_and_exactly_one_todo(ctx, kind):
    counts, has_gt = (17, 64, 5), (0, 0, 0)
    blocks = [(0, 1, False), (0, 2, False), (1, 2, False)]
    sides, arr, g = tsg.make_session(9500, counts, 0, has_gt, blocks, dict(GATE, skip_distance=np.inf))
    g = dict(g, desc_thresh=GATE["desc_thresh"])
    total = int(session_tables(counts, blocks)[2][-1])
    sim_in = given_similarity(None, total, g["desc_thresh"], kind)
    hip = Hip()
    try:
        got, tabs = run_gate_sim(ctx, hip, arr, counts, blocks, has_gt, g, sim_in)
        n = check_against_grid_gate_sim(ctx, hip, got, tabs, sides, counts, blocks, has_gt, g, sim_in, tag=kind)
        assert n == {"all": total, "none": 0, "one": 1}[kind]
        if kind == "one":
            assert got["pairs"][0].tolist() == [17 + 63, 17 + 64 + 4] and got["todo_off"].tolist() == [0, 0, 0, 1]
    finally:
        hip.free_all()


def test_a_descriptor_length_with_a_given_similarity_is_refused(ctx):
    counts, blocks = (3, 2), tsg.all_pairs(2)
    sides, arr, g = tsg.make_session(9600, counts, 0, (0, 0), blocks, GATE)
    tabs = session_tables(counts, blocks)
    with pytest.raises(_abi.RomanHipError) as e:
        ctx.session_gate(grid_gate_params(desc_dim=2, **g), *tabs, arr["pos"], arr["T_w"], time=arr["time"], sim_in=np.zeros(int(tabs[2][-1])))
    assert e.value.code == _abi.ROMAN_E_INVALID
    ctx.sync()
