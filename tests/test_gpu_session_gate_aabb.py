"""roman_session_gate_aabb_dev / roman_session_gate_aabb on the device against roman_grid_gate_aabb_dev called per
block on the SAME device: every dense value of a block BITWISE, flags included, the compact list of a block equal to that call's
pairs after re-basing with T_ref bitwise and enable equal, todo_off from the per-block counts, the capacity beyond the total
untouched.  Boxes are planted so that a pair touches exactly in one coordinate (NEARBY: the test is <= / >=), a pair is separated in
exactly one axis by one ulp, and a submap is empty (its infinite box is never NEARBY)."""
import numpy as np
import pytest

import _fill_boxes_oracle as fo
import _grid_gate_oracle as go
from _hipmem import Hip
from roman_amd.runtime import grid_gate_params, session_tables
from test_gpu_grid_gate import DTYPE, FILL, Guarded
from test_gpu_session_gate import OUT, WIDTH, all_pairs, session_arrays
from test_session_aabb_abi import check_boxes_error_codes, check_gate_error_codes

pytestmark = pytest.mark.gpu

GATE = dict(skip_distance=np.inf, desc_thresh=0.6, lc_time_thresh=60.0)


def make_session(seed, counts, d, blocks):
    """Sides per robot with ground-truth positions, and a box per global submap around its centre: integer corners, half widths of
    2 to 9 m in a 30 m box — some pairs intersect, some do not.  Then, in the first block that has both, robot r1's first boxes are
    planted against robot r0's first box: touching in x, one ulp apart in y and equal elsewhere, empty."""
    rng = np.random.default_rng(seed)
    sides = [go.random_side(rng, n, max(d, 1), box=30.0, with_gt=True) for n in counts]
    arr = session_arrays(sides, ("pos", "pos_gt", "T_w", "time"))
    arr["desc"] = np.concatenate([s["desc"].reshape(len(s["pos"]), d) for s in sides]) if d else None
    S = sum(counts)
    c, h = np.floor(arr["pos"]), rng.integers(2, 10, (S, 3)).astype(np.float64)
    box = np.hstack([c - h, c + h])
    sub_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    planted = {}
    for r0, r1, _ in blocks:
        if counts[r0] and counts[r1] and r0 != r1:
            a, g1 = box[sub_off[r0]].copy(), int(sub_off[r1])
            t = a.copy(); t[0] = a[3]; t[3] = a[3] + 3.0                      # min x of one = max x of the other
            box[g1] = t; planted["touch"] = (int(sub_off[r0]), g1)
            if counts[r1] > 1:
                u = a.copy(); u[1] = np.nextafter(a[4], np.inf); u[4] = a[4] + 3.0    # clear of it in y alone, by one ulp
                box[g1 + 1] = u; planted["ulp"] = (int(sub_off[r0]), g1 + 1)
            if counts[r1] > 2:
                box[g1 + 2] = [np.inf] * 3 + [-np.inf] * 3; planted["empty"] = (int(sub_off[r0]), g1 + 2)
            break
    near = fo.aabb_nearby(box, box)
    for kind, (gi, gj) in planted.items():
        assert near[gi, gj] == (kind == "touch"), kind
    if "empty" in planted:
        assert not near[:, planted["empty"][1]].any() and not near[planted["empty"][1]].any()
    return sides, arr, box, planted


def grid_aabb_dev(ctx, hip, a, b, box0, box1, gate, d, lc, sim_in=None):
    """roman_grid_gate_aabb_dev over guarded outputs -> dict of host arrays, compact arrays at full capacity."""
    S0, S1 = len(a["pos"]), len(b["pos"])
    B = S0 * S1
    up = lambda x: None if x is None or np.size(x) == 0 else hip.upload(np.asarray(x, dtype=np.float64).ravel())
    ins = [dict(pos=up(s["pos"]), gt=up(s["pos_gt"]), T_w=up(s["T_w"]), time=up(s["time"]), desc=up(s["desc"]) if d else None) for s in (a, b)]
    size = dict(dist=B, flags=B, yaw_deg=B, sim=B, T_ij=16 * B, pairs=2 * B, T_ref=16 * B, enable=B, n_todo=1)
    out = {k: Guarded(hip, n, DTYPE[k], FILL[k]) for k, n in size.items()}
    P = grid_gate_params(None, desc_dim=d, single_robot_lc=bool(lc), **gate)
    ctx.grid_gate_aabb_dev(P, S0, S1, ins[0]["pos"], ins[0]["T_w"], ins[1]["pos"], ins[1]["T_w"], *[out[k].ptr for k in size],
                           box0_ptr=up(box0), box1_ptr=up(box1), sim_in_ptr=up(sim_in), time0_ptr=ins[0]["time"], time1_ptr=ins[1]["time"],
                           desc0_ptr=ins[0]["desc"], desc1_ptr=ins[1]["desc"], pos_gt0_ptr=ins[0]["gt"], pos_gt1_ptr=ins[1]["gt"])
    ctx.sync()
    got = {k: v.get() for k, v in out.items()}
    got["pairs"] = got["pairs"].reshape(B, 2); got["T_ref"] = got["T_ref"].reshape(B, 4, 4)
    return got


def run_session(ctx, hip, arr, box, counts, blocks, has_gt, gate, d, sim_in=None, shift=0, use_gt=True):
    sub_off, blk, pair_off, tile_off = session_tables(counts, blocks)
    total, nb = int(pair_off[-1]), len(blocks)

    def up(x):
        if x is None or np.size(x) == 0:
            return None
        return hip.upload(np.concatenate([np.zeros(shift), np.asarray(x, dtype=np.float64).ravel()])) + 8 * shift
    out = {k: Guarded(hip, WIDTH[k] * total, DTYPE[k], FILL[k], shift) for k in OUT}
    out["todo_off"] = Guarded(hip, nb + 1, np.int32, -11, shift)
    P = grid_gate_params(None, desc_dim=d, single_robot_lc=False, **gate)       # (no radius: -1 is not read)
    ctx.session_gate_aabb_dev(P, sub_off, blk, pair_off, tile_off, hip.upload(sub_off), hip.upload(blk), hip.upload(pair_off), hip.upload(tile_off),
                              up(arr["pos"]), up(arr["T_w"]), *[out[k].ptr for k in OUT], out["todo_off"].ptr, up(box), time_ptr=up(arr["time"]),
                              desc_ptr=up(arr["desc"]) if d else None, pos_gt_ptr=up(arr["pos_gt"]) if use_gt else None,
                              has_gt_ptr=hip.upload(np.asarray(has_gt, dtype=np.int32)) if use_gt else None, sim_in_ptr=up(sim_in))
    ctx.sync()
    got = {k: v.get() for k, v in out.items()}
    got["T_ij"] = got["T_ij"].reshape(total, 4, 4); got["T_ref"] = got["T_ref"].reshape(total, 4, 4); got["pairs"] = got["pairs"].reshape(total, 2)
    return got, (sub_off, blk, pair_off, tile_off)


def check_blocks(ctx, hip, got, tabs, sides, box, counts, blocks, has_gt, gate, d, sim_in=None, tag=""):
    sub_off, _, pair_off, _ = tabs
    want_off = [0]
    for b, (r0, r1, lc) in enumerate(blocks):
        n0, n1 = counts[r0], counts[r1]
        lo, hi = int(pair_off[b]), int(pair_off[b + 1])
        if n0 == 0 or n1 == 0:
            want_off.append(want_off[-1]); continue
        gt = bool(has_gt[r0] and has_gt[r1])
        a, bb = dict(sides[r0]), dict(sides[r1])
        if not gt:
            a["pos_gt"] = bb["pos_gt"] = None
        if d == 0:
            a["desc"] = bb["desc"] = None
        one = grid_aabb_dev(ctx, hip, a, bb, box[sub_off[r0]:sub_off[r0 + 1]], box[sub_off[r1]:sub_off[r1 + 1]], gate, d, lc,
                            None if sim_in is None else sim_in[lo:hi])
        n = int(one["n_todo"][0])
        for k in ("dist", "flags", "yaw_deg", "sim", "T_ij"):              # (with sim_in neither call writes sim: the sentinel on both sides)
            assert got[k][lo:hi].tobytes() == one[k].tobytes(), (tag, blocks[b], k)
        s0, s1 = want_off[-1], want_off[-1] + n
        assert np.array_equal(got["pairs"][s0:s1], one["pairs"][:n] + np.array([sub_off[r0], sub_off[r1]], dtype=np.int32)), (tag, blocks[b], "pairs")
        assert got["T_ref"][s0:s1].tobytes() == one["T_ref"][:n].tobytes(), (tag, blocks[b], "T_ref")
        assert np.array_equal(got["enable"][s0:s1], one["enable"][:n]), (tag, blocks[b], "enable")
        want_off.append(s1)
    assert got["todo_off"].tolist() == want_off, (tag, got["todo_off"].tolist(), want_off)
    n = want_off[-1]
    assert (got["pairs"][n:] == FILL["pairs"]).all() and (got["T_ref"][n:] == FILL["T_ref"]).all() and (got["enable"][n:] == FILL["enable"]).all(), \
        (tag, "capacity slots beyond the total were written")
    return n


def nearby_of(got, tabs, counts, blocks):
    """-> the NEARBY bit of every pair of every block as (gi, gj) -> bool."""
    sub_off, _, pair_off, _ = tabs
    out = {}
    for b, (r0, r1, _) in enumerate(blocks):
        f = got["flags"][int(pair_off[b]):int(pair_off[b + 1])].reshape(counts[r0], counts[r1])
        for i in range(counts[r0]):
            for j in range(counts[r1]):
                out[(int(sub_off[r0]) + i, int(sub_off[r1]) + j)] = bool(f[i, j] & go.NEARBY)
    return out


COUNTS = [(1,), (1, 1), (3, 0, 5), (5, 3, 6), (17, 64, 5), (65, 63)]
VARIANTS = [(0, False), (1, False), (16, False), (769, False), (0, True)]       # (descriptor length, the similarity is given)


@pytest.mark.parametrize("d,given", VARIANTS, ids=[f"d{d}" + ("-sim_in" if g else "") for d, g in VARIANTS])
@pytest.mark.parametrize("counts", COUNTS, ids=["-".join(map(str, c)) for c in COUNTS])
def test_blocks_equal_grid_gate_aabb_dev_bitwise(ctx, counts, d, given):
    """All r <= s (self_lc on the diagonal blocks); ground truth on none / one / all robots, a finite skip distance and shifted
    buffers alternate over the cases."""
    v = COUNTS.index(counts) + VARIANTS.index((d, given))
    R = len(counts)
    has_gt = [[0] * R, [1] + [0] * (R - 1), [1] * R][v % 3]
    blocks = all_pairs(R)
    gate = dict(GATE, skip_distance=[np.inf, 25.0][v % 2], desc_thresh=0.6 if (d or given) else 0.0)
    sides, arr, box, planted = make_session(9100 + 10 * COUNTS.index(counts) + VARIANTS.index((d, given)), counts, d, blocks)
    total = int(session_tables(counts, blocks)[2][-1])
    sim_in = np.random.default_rng(v).uniform(0.2, 0.95, total) if given else None
    if given:
        sim_in[::7] = 0.6                                    # equal to the threshold: passes
    hip = Hip()
    try:
        got, tabs = run_session(ctx, hip, arr, box, counts, blocks, has_gt, gate, d, sim_in, shift=v % 2)
        n = check_blocks(ctx, hip, got, tabs, sides, box, counts, blocks, has_gt, gate, d, sim_in, tag=f"{counts} d={d} given={given}")
        near = nearby_of(got, tabs, counts, blocks)
        for kind, key in planted.items():
            assert near[key] == (kind == "touch"), (kind, key)
        if len(counts) > 1 and min(c for c in counts if c) > 2:
            assert any(near.values()) and not all(near.values())
        assert np.array_equal(np.isnan(got["yaw_deg"]), (got["flags"] & go.NEARBY) == 0)     # the yaw of NEARBY pairs only
        if given:
            assert (got["sim"] == FILL["sim"]).all()         # sim is not written when the similarity is given
        print(f"{counts} d={d} given={given}: {n} of {total} pairs TODO, {sum(near.values())} NEARBY, planted {sorted(planted)}")
    finally:
        hip.free_all()


@pytest.mark.parametrize("kind", ["all", "none", "one_in_the_last_block", "self_lc_on_some"])
def test_todo_extremes_and_per_block_self_lc(ctx, kind):
    counts = (17, 64, 5)
    blocks = {"all": all_pairs(3), "none": [b for b in all_pairs(3) if b[0] != b[1]], "one_in_the_last_block": [(0, 1, False), (0, 2, False), (1, 2, False)],
              "self_lc_on_some": [(0, 0, True), (1, 1, False), (0, 2, False), (2, 0, True), (2, 2, True)]}[kind]
    sides, arr, box, _ = make_session(9400, counts, 0, blocks)
    if kind == "one_in_the_last_block":                      # two submaps at one place in the last block
        sides[2]["pos"][4] = sides[1]["pos"][63]
        arr = dict(session_arrays(sides, ("pos", "pos_gt", "T_w", "time")), desc=None)
    gate = dict(GATE, desc_thresh=0.0, skip_distance=np.inf if kind in ("all", "self_lc_on_some") else 1e-3)
    hip = Hip()
    try:
        got, tabs = run_session(ctx, hip, arr, box, counts, blocks, (0, 0, 0), gate, 0, use_gt=False)
        n = check_blocks(ctx, hip, got, tabs, sides, box, counts, blocks, (0, 0, 0), gate, 0, tag=kind)
        total = int(tabs[2][-1])
        if kind != "self_lc_on_some":
            assert n == {"all": total, "none": 0, "one_in_the_last_block": 1}[kind]
        if kind == "one_in_the_last_block":
            assert got["pairs"][0].tolist() == [17 + 63, 17 + 64 + 4] and got["todo_off"].tolist() == [0, 0, 0, 1]
        if kind == "self_lc_on_some":                        # the time gate follows each block's own flag
            en, off = got["enable"], got["todo_off"]
            assert (en[off[1]:off[3]] == 1).all() and (en[off[0]:off[1]] == 0).any() and (en[off[4]:off[5]] == 0).any() and n == off[-1]
    finally:
        hip.free_all()


def test_two_runs_agree_bitwise_and_host_pointers_agree_with_device_pointers(ctx):
    counts, d, has_gt, blocks = (17, 64, 5), 769, (1, 1, 0), all_pairs(3)
    sides, arr, box, _ = make_session(9500, counts, d, blocks)
    hip = Hip()
    try:
        a, tabs = run_session(ctx, hip, arr, box, counts, blocks, has_gt, GATE, d)
        b, _ = run_session(ctx, hip, arr, box, counts, blocks, has_gt, GATE, d, shift=1)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        total = int(tabs[2][-1])
        given = dict(pairs=np.full((total, 2), FILL["pairs"], np.int32), T_ref=np.full((total, 4, 4), FILL["T_ref"]), enable=np.full(total, FILL["enable"], np.int32))
        h = ctx.session_gate_aabb(grid_gate_params(None, desc_dim=d, **GATE), box, *tabs, arr["pos"], arr["T_w"], time=arr["time"], desc=arr["desc"],
                                  pos_gt=arr["pos_gt"], has_gt=has_gt, **given)
        for k in ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert np.asarray(getattr(h, k)).tobytes() == a[k].tobytes(), k          # (the untouched capacity included: inout)
        sim_in = np.random.default_rng(3).uniform(0.2, 0.95, total)
        c, _ = run_session(ctx, hip, arr, box, counts, blocks, has_gt, GATE, 0, sim_in)
        h = ctx.session_gate_aabb(grid_gate_params(None, desc_dim=0, **GATE), box, *tabs, arr["pos"], arr["T_w"], time=arr["time"], pos_gt=arr["pos_gt"],
                                  has_gt=has_gt, sim_in=sim_in, **given)
        for k in ("dist", "flags", "yaw_deg", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert np.asarray(getattr(h, k)).tobytes() == c[k].tobytes(), k
        assert np.array_equal(h.sim, sim_in)
    finally:
        hip.free_all()


def test_error_codes(ctx):
    check_boxes_error_codes(ctx._lib, ctx._h)
    check_gate_error_codes(ctx._lib, ctx._h)
