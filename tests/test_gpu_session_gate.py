"""roman_session_gate_dev / roman_session_gate on the device against roman_grid_gate_dev called per block on the
SAME device: every dense value of a block BITWISE, the compact list of a block equal to that call's pairs mapped to global indices
with T_ref bitwise and enable equal, todo_off from the per-block counts.  Generated inputs carry no borderline flag
(tests/_grid_gate_oracle.borderline: a flagged seed is an error, never a skip)."""
import numpy as np
import pytest

import _grid_gate_oracle as go
import _session as ss
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import grid_gate_params, session_tables
from test_gpu_grid_gate import DTYPE, FILL, Guarded, close, run_dev
from test_session_abi import check_error_codes

pytestmark = pytest.mark.gpu

OUT = ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable")
WIDTH = dict(dist=1, flags=1, yaw_deg=1, sim=1, T_ij=16, pairs=2, T_ref=16, enable=1)
GATE = dict(radius=12.0, skip_distance=np.inf, desc_thresh=0.6, lc_time_thresh=60.0)


def all_pairs(R):
    return [(r, s, r == s) for r in range(R) for s in range(r, R)]


def session_arrays(sides, keys):
    """The robots' arrays one behind the other (a robot without submaps adds nothing)."""
    tail = dict(pos=(3,), pos_gt=(3,), T_w=(16,), time=())
    return {k: np.concatenate([np.asarray(s[k], dtype=np.float64).reshape((len(s["pos"]),) + tail[k]) for s in sides]) for k in keys}


def make_session(seed, counts, d, has_gt, blocks, gate, box=30.0):
    """Sides per robot (ground truth positions for all: has_gt decides who uses them), checked clean for every block."""
    rng = np.random.default_rng(seed)
    sides = [go.random_side(rng, n, max(d, 1), box=box, with_gt=True) for n in counts]
    g = dict(gate); g["desc_thresh"] = g["desc_thresh"] if d else 0.0
    for r0, r1, lc in blocks:
        if counts[r0] and counts[r1]:
            gt = bool(has_gt[r0] and has_gt[r1])
            a, b = dict(sides[r0]), dict(sides[r1])
            if not gt:
                a["pos_gt"] = b["pos_gt"] = None
            if d == 0:
                a["desc"] = b["desc"] = None
            assert not go.borderline(a, b, single_robot_lc=bool(lc), **g), f"seed {seed} gives a borderline block {(r0, r1)}: choose another seed"
    arr = session_arrays(sides, ("pos", "pos_gt", "T_w", "time"))
    arr["desc"] = np.concatenate([s["desc"].reshape(len(s["pos"]), d) for s in sides]) if d else None
    return sides, arr, g


def run_session_dev(ctx, hip, arr, counts, blocks, has_gt, gate, d, shift=0, use_gt=True):
    sub_off, blk, pair_off, tile_off = session_tables(counts, blocks)
    total, nb = int(pair_off[-1]), len(blocks)

    def up(x):
        if x is None or x.size == 0:
            return None
        return hip.upload(np.concatenate([np.zeros(shift), np.asarray(x, dtype=np.float64).ravel()])) + 8 * shift
    out = {k: Guarded(hip, WIDTH[k] * total, DTYPE[k], FILL[k], shift) for k in OUT}
    out["todo_off"] = Guarded(hip, nb + 1, np.int32, -11, shift)
    P = grid_gate_params(desc_dim=d, single_robot_lc=False, **gate)
    ctx.session_gate_dev(P, sub_off, blk, pair_off, tile_off, hip.upload(sub_off), hip.upload(blk), hip.upload(pair_off), hip.upload(tile_off),
                         up(arr["pos"]), up(arr["T_w"]), *[out[k].ptr for k in OUT], out["todo_off"].ptr, time_ptr=up(arr["time"]),
                         desc_ptr=up(arr["desc"]) if d else None, pos_gt_ptr=up(arr["pos_gt"]) if use_gt else None,
                         has_gt_ptr=hip.upload(np.asarray(has_gt, dtype=np.int32)) if use_gt else None)
    ctx.sync()
    got = {k: v.get() for k, v in out.items()}
    for k in ("T_ij", "T_ref"):
        got[k] = got[k].reshape(total, 4, 4)
    got["pairs"] = got["pairs"].reshape(total, 2)
    return got, (sub_off, blk, pair_off, tile_off)


def check_against_grid_gate(ctx, hip, got, tabs, sides, counts, blocks, has_gt, gate, d, tag=""):
    """Block by block against roman_grid_gate_dev on the block's two sides, same device."""
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
        one = run_dev(ctx, hip, a, bb, dict(single_robot_lc=bool(lc), **gate))
        n = int(one["n_todo"][0])
        for k in ("dist", "flags", "yaw_deg", "sim", "T_ij"):
            assert got[k][lo:hi].tobytes() == one[k].reshape(got[k][lo:hi].shape).tobytes(), (tag, blocks[b], k)
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


COUNTS = [(1,), (1, 1), (3, 0, 5), (5, 3, 6), (17, 64, 5), (65, 63), (32, 32)]
DIMS = [0, 1, 16, 769]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("counts", COUNTS, ids=["-".join(map(str, c)) for c in COUNTS])
def test_blocks_equal_grid_gate_dev_bitwise(ctx, counts, d):
    """All r <= s; ground truth on none / some / all robots, a finite skip distance and shifted buffers alternate over the cases.
    (32, 32): blocks of exactly 1024 pairs — every block boundary on a scan workgroup's boundary; (5, 3, 6): a block ends inside a
    tile and inside a workgroup; (17, 64, 5) and (65, 63): more than 2 x 1024 flags."""
    v = COUNTS.index(counts) + DIMS.index(d)
    R = len(counts)
    has_gt = [[0] * R, [1] + [0] * (R - 1), [1] * R][v % 3]
    blocks = all_pairs(R)
    gate = dict(GATE, skip_distance=[np.inf, 25.0][v % 2])
    sides, arr, g = make_session(8100 + 10 * COUNTS.index(counts) + DIMS.index(d), counts, d, has_gt, blocks, gate)
    hip = Hip()
    try:
        got, tabs = run_session_dev(ctx, hip, arr, counts, blocks, has_gt, g, d, shift=v % 2)
        n = check_against_grid_gate(ctx, hip, got, tabs, sides, counts, blocks, has_gt, g, d, tag=f"{counts} d={d}")
        print(f"{counts} d={d}: {n} of {int(tabs[2][-1])} pairs TODO")
    finally:
        hip.free_all()


LISTS = dict(one_block=[(1, 2, False)], off_diagonal=[(0, 1, False), (0, 2, False), (1, 2, False)],
             reversed=list(reversed(all_pairs(3))), self_lc_on_some=[(0, 0, True), (1, 1, False), (0, 2, False), (2, 0, True), (2, 2, True)])


@pytest.mark.parametrize("name", sorted(LISTS))
def test_block_lists(ctx, name):
    """Other lists than all r <= s; `self_lc_on_some`: the time gate follows each block's own flag (times on both sides of the
    threshold: the generated times spread over ten minutes, the threshold is one)."""
    counts, d, blocks = (5, 3, 6), 16, LISTS[name]
    sides, arr, g = make_session(8300 + sorted(LISTS).index(name), counts, d, (1, 0, 1), blocks, GATE)
    hip = Hip()
    try:
        got, tabs = run_session_dev(ctx, hip, arr, counts, blocks, (1, 0, 1), g, d)
        n = check_against_grid_gate(ctx, hip, got, tabs, sides, counts, blocks, (1, 0, 1), g, d, tag=name)
        if name == "self_lc_on_some":
            en, off = got["enable"], got["todo_off"]
            assert (en[off[1]:off[3]] == 1).all() and (en[off[0]:off[1]] == 0).any() and (en[off[4]:off[5]] == 0).any() and n == off[-1]
    finally:
        hip.free_all()


@pytest.mark.parametrize("kind", ["all", "none", "one_in_the_last_block"])
def test_all_none_and_exactly_one_todo(ctx, kind):
    counts, blocks = (17, 64, 5), all_pairs(3)
    gate = dict(GATE, skip_distance={"all": np.inf, "none": 1e-3, "one_in_the_last_block": 1e-3}[kind])
    rng = np.random.default_rng(8400)
    sides = [go.random_side(rng, n, 1, with_gt=False) for n in counts]
    if kind == "none":                                       # every pair beyond the skip distance: also a submap against itself
        blocks = [b for b in blocks if b[0] != b[1]]
    if kind == "one_in_the_last_block":                      # off-diagonal blocks, and two submaps at one place in the last of them
        blocks = [(0, 1, False), (0, 2, False), (1, 2, False)]
        sides[2]["pos"][4] = sides[1]["pos"][63]
    for s in sides:
        s["desc"] = None
    arr = session_arrays(sides, ("pos", "T_w", "time"))
    arr["desc"] = None; arr["pos_gt"] = None
    g = dict(gate, desc_thresh=0.0)
    hip = Hip()
    try:
        got, tabs = run_session_dev(ctx, hip, arr, counts, blocks, (0, 0, 0), g, 0, use_gt=False)
        n = check_against_grid_gate(ctx, hip, got, tabs, sides, counts, blocks, (0, 0, 0), g, 0, tag=kind)
        assert n == {"all": int(tabs[2][-1]), "none": 0, "one_in_the_last_block": 1}[kind]
        if kind == "one_in_the_last_block":
            assert got["pairs"][0].tolist() == [17 + 63, 17 + 64 + 4] and got["todo_off"].tolist() == [0, 0, 0, 1]
    finally:
        hip.free_all()


def test_two_runs_agree_bitwise_and_host_pointers_agree_with_device_pointers(ctx):
    counts, d, has_gt, blocks = (17, 64, 5), 769, (1, 1, 0), all_pairs(3)
    sides, arr, g = make_session(8500, counts, d, has_gt, blocks, GATE)
    hip = Hip()
    try:
        a, tabs = run_session_dev(ctx, hip, arr, counts, blocks, has_gt, g, d)
        b, _ = run_session_dev(ctx, hip, arr, counts, blocks, has_gt, g, d, shift=1)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        total = int(tabs[2][-1])
        given = dict(pairs=np.full((total, 2), FILL["pairs"], np.int32), T_ref=np.full((total, 4, 4), FILL["T_ref"]), enable=np.full(total, FILL["enable"], np.int32))
        h = ctx.session_gate(grid_gate_params(desc_dim=d, **g), *tabs, arr["pos"], arr["T_w"], time=arr["time"], desc=arr["desc"], pos_gt=arr["pos_gt"],
                             has_gt=has_gt, **given)
        for k in ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert np.asarray(getattr(h, k)).tobytes() == a[k].tobytes(), k          # (the untouched capacity included: inout)
    finally:
        hip.free_all()


def check_against_numpy(o, got, tag):
    """A session result against a NumPy restatement: what tests/test_gpu_grid_gate.check() holds exact is exact here."""
    n = int(o["todo_off"][-1])
    assert np.asarray(got["todo_off"]).tolist() == o["todo_off"].tolist(), tag
    assert np.array_equal(got["flags"], o["flags"]), tag
    assert np.array_equal(got["pairs"][:n], o["pairs"]) and np.array_equal(got["enable"][:n], o["enable"]), tag
    for k in ("dist", "sim", "yaw_deg", "T_ij"):
        assert close(got[k], o[k]), (tag, k)
    assert close(got["T_ref"][:n], o["T_ref"]), tag
    assert got["T_ref"][:n].tobytes() == got["T_ij"][(o["flags"] & go.TODO) != 0].tobytes(), (tag, "T_ref is not the pair's T_ij")
    assert (got["pairs"][n:] == FILL["pairs"]).all() and (got["T_ref"][n:] == FILL["T_ref"]).all() and (got["enable"][n:] == FILL["enable"]).all(), \
        (tag, "capacity slots beyond the total were written")


@pytest.mark.parametrize("entry", ["session_gate", "session_gate_sim", "session_gate_aabb", "session_gate_aabb-sim_in"])
def test_every_entry_against_the_numpy_restatement(ctx, entry):
    """Each of the six entry points, host and `_dev`, against tests/_session.py / tests/_session_aabb.py on two robots of 2 and 5
    submaps, a block (0, 1) and a self block (1, 1), ground truth on robot 0 only (so pos is what is read, never pos_gt): an entry
    that hands the gate one array for another of its type — pos_gt for pos, sim for sim_in, T_ref for T_ij — misses it."""
    import _session_aabb as sa
    import _session_stacked as sst
    aabb, given = "aabb" in entry, "sim" in entry
    counts, blocks, has_gt = (2, 5), [(0, 1, False), (1, 1, True)], (1, 0)
    sides, arr, g = make_session(8700, counts, 3, has_gt, blocks, GATE)
    rng = np.random.default_rng(8701)
    box = np.hstack([arr["pos"] - rng.uniform(5.0, 25.0, (7, 3)), arr["pos"] + rng.uniform(5.0, 25.0, (7, 3))])
    sim_in = rng.uniform(0.2, 0.95, 35)
    tabs = session_tables(counts, blocks)
    sub_off, blk, pair_off, _ = tabs
    rest = {k: g[k] for k in ("skip_distance", "desc_thresh", "lc_time_thresh")}
    seen = dict(arr, desc=None) if given else arr
    if aabb:
        o = sa.session_gate_aabb_oracle(seen, box, sub_off, blk, has_gt, sim_in=sim_in if given else None, pair_off=pair_off, **rest)
    else:
        o = ss.session_gate_oracle(seen, sub_off, blk, has_gt, g["radius"], **rest)
        if given:
            o = {**o, **sst.gate_from_sim(o, sim_in, sub_off, blk, g["desc_thresh"], arr["time"], g["lc_time_thresh"]), "sim": sim_in}
    n = int(o["todo_off"][-1])
    assert 0 < n < 35 and set(o["enable"].tolist()) == {0, 1} and 0 < ((o["flags"] & go.NEARBY) != 0).sum() < 35, "the case lost its classes"
    P = grid_gate_params(None if aabb else g["radius"], desc_dim=0 if given else 3, single_robot_lc=False, **rest)
    hip = Hip()
    try:
        up = lambda x: hip.upload(np.asarray(x, dtype=np.float64).ravel())
        out = {k: Guarded(hip, WIDTH[k] * 35, DTYPE[k], FILL[k]) for k in OUT}
        out["todo_off"] = Guarded(hip, 3, np.int32, -11)
        ctx.session_gate_dev(P, *tabs, *[hip.upload(t) for t in tabs], up(arr["pos"]), up(arr["T_w"]), *[out[k].ptr for k in OUT], out["todo_off"].ptr,
                             time_ptr=up(arr["time"]), desc_ptr=None if given else up(arr["desc"]), pos_gt_ptr=up(arr["pos_gt"]),
                             has_gt_ptr=hip.upload(np.asarray(has_gt, dtype=np.int32)), sim_in_ptr=up(sim_in) if given else None,
                             box_ptr=up(box) if aabb else None)
        ctx.sync()
        got = {k: v.get() for k, v in out.items()}
        if given:                                              # an entry that is given the similarity does not write one
            assert (got["sim"] == FILL["sim"]).all()
            got["sim"] = sim_in
        got["T_ij"] = got["T_ij"].reshape(35, 4, 4); got["T_ref"] = got["T_ref"].reshape(35, 4, 4); got["pairs"] = got["pairs"].reshape(35, 2)
        check_against_numpy(o, got, entry + "_dev")
        handed = dict(pairs=np.full((35, 2), FILL["pairs"], np.int32), T_ref=np.full((35, 4, 4), FILL["T_ref"]), enable=np.full(35, FILL["enable"], np.int32))
        h = ctx.session_gate(P, *tabs, arr["pos"], arr["T_w"], time=arr["time"], desc=None if given else arr["desc"], pos_gt=arr["pos_gt"], has_gt=has_gt,
                             sim_in=sim_in if given else None, box=box if aabb else None, **handed)
        check_against_numpy(o, {k: np.asarray(getattr(h, k)) for k in OUT + ("todo_off",)}, entry)
    finally:
        hip.free_all()


def test_empty_sessions(ctx):
    hip = Hip()
    try:
        for counts, blocks in (((3, 2), []), ((0, 4, 0), [(0, 1, False), (0, 0, True), (1, 2, False)])):
            sides, arr, g = make_session(8600, counts, 0, [0] * len(counts), blocks, GATE)
            got, tabs = run_session_dev(ctx, hip, arr, counts, blocks, [0] * len(counts), g, 0, use_gt=False)
            assert got["todo_off"].tolist() == [0] * (len(blocks) + 1) and tabs[2][-1] == 0
            h = ctx.session_gate(grid_gate_params(**g), *tabs, arr["pos"], arr["T_w"], time=arr["time"])
            assert h.todo_off.tolist() == [0] * (len(blocks) + 1)
    finally:
        hip.free_all()


def test_error_codes(ctx):
    check_error_codes(ctx._lib, ctx._h)
