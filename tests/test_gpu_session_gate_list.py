"""roman_session_gate_list_dev / roman_session_gate_list on the device against roman_session_gate_dev /
roman_session_gate_sim_dev / roman_session_gate_aabb_dev over the SAME tables on the SAME device: entry l of every per-pair output
BITWISE what the whole-grid call writes at the pair's dense position, the compact list the TODO pairs in list order with T_ref
bitwise and enable equal, todo_off from the listed pairs' blocks.  The whole-grid run of a case is made once and shared by all
its lists."""
import numpy as np
import pytest

import _grid_gate_oracle as go
from _hipmem import Hip
from roman_amd.runtime import grid_gate_params, session_pair_list, session_tables
from test_gpu_grid_gate import DTYPE, FILL, Guarded
from test_session_update_abi import check_error_codes

pytestmark = pytest.mark.gpu

OUT = ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable")
WIDTH = dict(dist=1, flags=1, yaw_deg=1, sim=1, T_ij=16, pairs=2, T_ref=16, enable=1)
GATE = dict(radius=12.0, skip_distance=25.0, desc_thresh=0.6, lc_time_thresh=60.0)
COUNTS = [(1,), (3, 0, 5), (17, 64, 5)]
DIMS = [0, 1, 16, 769]
LENGTHS = (3, 4, 5, 63, 64, 65, 1025)       # the four-entry wave, a wave of flags, the 1024-flag workgroup of the count kernel


def all_pairs(R):
    return [(r, s, r == s) for r in range(R) for s in range(r, R)]


class Session:
    """Generated arrays of one session on the device, and the whole-grid gate over them as the expectation."""

    def __init__(self, ctx, hip, seed, counts, d, blocks, has_gt=None, gate=GATE, mode="radius", arrays=None, sim_in=None):
        self.ctx, self.hip, self.counts, self.d, self.blocks, self.mode = ctx, hip, counts, d, blocks, mode
        rng = np.random.default_rng(seed)
        S, R = int(sum(counts)), len(counts)
        side = arrays or go.random_side(rng, S, max(d, 1), box=30.0, with_gt=True)
        self.arr = {k: np.asarray(side[k], dtype=np.float64) for k in ("pos", "pos_gt", "T_w", "time")}
        self.arr["desc"] = np.asarray(side["desc"], dtype=np.float64).reshape(S, d) if d and mode != "sim" and mode != "aabb-sim" else None
        self.has_gt = None if has_gt is None else np.asarray(has_gt, dtype=np.int32)
        self.tabs = session_tables(counts, blocks)
        self.sub_off, self.blk, self.pair_off, self.tile_off = self.tabs
        self.total, self.nb = int(self.pair_off[-1]), len(blocks)
        self.box = np.hstack([self.arr["pos"] - rng.uniform(5.0, 25.0, (S, 3)), self.arr["pos"] + rng.uniform(5.0, 25.0, (S, 3))]) if "aabb" in mode else None
        self.sim_in = (rng.uniform(0.2, 0.95, self.total) if sim_in is None else sim_in) if "sim" in mode else None
        self.gd = 0 if "sim" in mode else d
        g = dict(gate); g["desc_thresh"] = g["desc_thresh"] if (d or "sim" in mode) else 0.0
        self.P = grid_gate_params(desc_dim=self.gd, single_robot_lc=False, **g)
        self.full_list = np.array([(b, i, j) for b, (r0, r1, _) in enumerate(blocks) for i in range(counts[r0]) for j in range(counts[r1])],
                                  dtype=np.int32).reshape(-1, 3)
        self.dev = {}
        self.full = self.run_full()

    def up(self, x, shift=0):
        if x is None or np.size(x) == 0:
            return None
        return self.hip.upload(np.concatenate([np.zeros(shift), np.asarray(x, dtype=np.float64).ravel()])) + 8 * shift

    def inputs(self, shift):
        if shift not in self.dev:
            a = self.arr
            self.dev[shift] = dict(tabs=[self.hip.upload(t) for t in self.tabs], pos=self.up(a["pos"], shift), T_w=self.up(a["T_w"], shift),
                                   kw=dict(time_ptr=self.up(a["time"], shift), desc_ptr=self.up(a["desc"], shift),
                                           pos_gt_ptr=None if self.has_gt is None else self.up(a["pos_gt"], shift),
                                           has_gt_ptr=None if self.has_gt is None else self.hip.upload(self.has_gt),
                                           sim_in_ptr=self.up(self.sim_in, shift), box_ptr=self.up(self.box, shift)))
        return self.dev[shift]

    def outputs(self, n, shift):
        out = {k: Guarded(self.hip, WIDTH[k] * n, DTYPE[k], FILL[k], shift) for k in OUT}
        out["todo_off"] = Guarded(self.hip, self.nb + 1, np.int32, -11, shift)
        return out

    @staticmethod
    def fetch(out, n):
        got = {k: v.get() for k, v in out.items()}
        got["T_ij"] = got["T_ij"].reshape(n, 16); got["T_ref"] = got["T_ref"].reshape(n, 16); got["pairs"] = got["pairs"].reshape(n, 2)
        return got

    def run_full(self):
        i, out = self.inputs(0), self.outputs(self.total, 0)
        self.ctx.session_gate_dev(self.P, *self.tabs, *i["tabs"], i["pos"], i["T_w"], *[out[k].ptr for k in OUT], out["todo_off"].ptr, **i["kw"])
        self.ctx.sync()
        got = self.fetch(out, self.total)
        if self.sim_in is not None:
            got["sim"] = self.sim_in.copy()
        return got

    def run_list(self, lst, shift=0):
        i, L = self.inputs(shift), len(lst)
        out = self.outputs(L, shift)
        self.ctx.session_gate_list_dev(self.P, *self.tabs[:3], lst, *i["tabs"][:3], self.hip.upload(lst), i["pos"], i["T_w"],
                                       *[out[k].ptr for k in OUT], out["todo_off"].ptr, **i["kw"])
        self.ctx.sync()
        return self.fetch(out, L)

    def expected(self, lst):
        """What the list call must write, from the whole-grid run: -> (per-pair outputs, compact outputs up to the total, todo_off)."""
        f, blk = self.full, self.blk
        n1 = np.array([self.counts[r1] for _, r1, _ in self.blocks], dtype=np.int64)
        b, i, j = (lst[:, k].astype(np.int64) for k in range(3))
        idx = self.pair_off[b] + i * n1[b] + j if len(lst) else np.zeros(0, dtype=np.int64)
        dense = {k: f[k][idx] for k in ("dist", "flags", "yaw_deg", "sim", "T_ij")}
        todo = (dense["flags"] & go.TODO) != 0
        rank = np.cumsum((f["flags"] & go.TODO) != 0) - 1              # the compact slot of a dense TODO pair in the whole-grid run
        compact = dict(pairs=np.stack([self.sub_off[blk[b, 0]] + i, self.sub_off[blk[b, 1]] + j], axis=1)[todo].astype(np.int32),
                       T_ref=dense["T_ij"][todo], enable=f["enable"][rank[idx[todo]]])
        todo_off = np.concatenate([[0], np.cumsum(np.bincount(b[todo], minlength=self.nb))]).astype(np.int32)
        return dense, compact, todo_off

    def check(self, lst, got, tag):
        lst = np.asarray(lst, dtype=np.int32).reshape(-1, 3)
        dense, compact, todo_off = self.expected(lst)
        n = int(todo_off[-1])
        assert got["todo_off"].tolist() == todo_off.tolist(), (tag, got["todo_off"].tolist(), todo_off.tolist())
        for k, want in dense.items():
            assert got[k].tobytes() == np.ascontiguousarray(want).tobytes(), (tag, k)
        for k, want in compact.items():
            assert got[k][:n].tobytes() == np.ascontiguousarray(want).tobytes(), (tag, k)
            assert (got[k][n:] == FILL[k]).all(), (tag, k, "capacity slots beyond the total were written")
        return n


def lists_of(s, rng):
    """name -> list, for a session of any size: what the session's pairs allow of the issue's lists."""
    F, T = s.full_list, s.total
    out = dict(empty=F[:0], one=F[T // 2:T // 2 + 1], full=F, every_fourth=F[::4])
    out["l_shape"] = session_pair_list(s.counts, s.blocks, [np.arange(n) == n - 1 for n in s.counts])
    for n in LENGTHS:
        if n <= T:
            out[f"random_{n}"] = F[np.sort(rng.choice(T, n, replace=False))]
            out[f"run_{n}"] = F[(T - n) // 2:(T - n) // 2 + n]                  # consecutive pairs: the groups of four cross row ends
    live = [b for b in range(s.nb) if s.pair_off[b + 1] > s.pair_off[b]]
    if len(live) > 1:                                                       # four-entry groups across a row end and a block end
        e = int(s.pair_off[live[0] + 1])
        out["straddle_block_end"] = F[max(e - 6, 0):e + 5]
        out["straddle_block_end_odd"] = F[max(e - 3, 0):e + 2]
    if len(live) > 2:                                                       # blocks without a listed pair in front, between and behind
        keep = np.isin(F[:, 0], live[1:-1:2])
        out["inner_blocks_only"] = F[keep][::3]
        out["last_block_only"] = F[F[:, 0] == live[-1]]
        out["first_block_only"] = F[F[:, 0] == live[0]][1::2]
    return out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("counts", COUNTS, ids=["-".join(map(str, c)) for c in COUNTS])
def test_lists_equal_the_whole_grid_gate_bitwise(ctx, counts, d):
    """All r <= s with self_lc on the self blocks; ground truth on none / one / all robots and shifted buffers alternate."""
    v = COUNTS.index(counts) + DIMS.index(d)
    R = len(counts)
    has_gt = [None, [1] + [0] * (R - 1), [1] * R][v % 3]
    hip = Hip()
    try:
        s = Session(ctx, hip, 9100 + v, counts, d, all_pairs(R), has_gt)
        lists = lists_of(s, np.random.default_rng(9200 + v))
        todo = {}
        for k, (name, lst) in enumerate(lists.items()):
            todo[name] = s.check(lst, s.run_list(lst, shift=(k + v) % 2), f"{counts} d={d} {name}")
        full = s.run_list(s.full_list)
        for k in OUT + ("todo_off",):                            # the full list: every output is the whole-grid call's
            assert full[k].tobytes() == s.full[k].tobytes() or (k == "sim" and s.sim_in is not None), k
        print(f"{counts} d={d}: TODO per list {todo}")
    finally:
        hip.free_all()


@pytest.mark.parametrize("mode", ["sim", "aabb", "aabb-sim"])
def test_given_similarity_and_bounding_boxes(ctx, mode):
    hip = Hip()
    try:
        for counts in COUNTS[1:]:
            s = Session(ctx, hip, 9300 + counts[0], counts, 16, all_pairs(len(counts)), [1] * len(counts), mode=mode)
            near = (s.full["flags"] & go.NEARBY) != 0
            assert 0 < near.sum() < s.total, "the case lost its classes"
            for name, lst in lists_of(s, np.random.default_rng(9301)).items():
                s.check(lst, s.run_list(lst), f"{mode} {counts} {name}")
    finally:
        hip.free_all()


def test_similarity_at_the_threshold(ctx):
    """sim_in at, just below and just above the threshold, and -inf: equality passes, everything below is gated."""
    counts, blocks = (3, 0, 5), all_pairs(3)
    total = int(session_tables(counts, blocks)[2][-1])
    t = GATE["desc_thresh"]
    special = np.array([t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), -np.inf])
    sim_in = np.tile(special, (total + 3) // 4)[:total]
    hip = Hip()
    try:
        s = Session(ctx, hip, 9400, counts, 0, blocks, None, gate=dict(GATE, skip_distance=np.inf), mode="sim", sim_in=sim_in)
        for name, cut in (("odd", slice(1, None, 2)), ("even", slice(0, None, 2)), ("every_third", slice(0, None, 3))):
            lst, want = s.full_list[cut], sim_in[cut]            # (the full list is in dense order)
            got = s.run_list(lst)
            s.check(lst, got, "threshold " + name)
            assert got["sim"].tobytes() == want.tobytes(), name
            gated, todo = (got["flags"] & go.GATED) != 0, (got["flags"] & go.TODO) != 0
            assert np.array_equal(gated, want < t) and np.array_equal(todo, want >= t), name         # (nothing is skipped: no skip distance)
            assert {"odd": gated.all(), "even": todo.all(), "every_third": gated.any() and todo.any()}[name]
    finally:
        hip.free_all()


@pytest.mark.parametrize("kind", ["all", "none", "one"])
def test_all_none_and_exactly_one_todo(ctx, kind):
    counts, blocks = (17, 64, 5), [(0, 1, False), (0, 2, False), (1, 2, False)]
    rng = np.random.default_rng(9500)
    side = go.random_side(rng, sum(counts), 1, with_gt=False)
    if kind == "one":                                        # two submaps at one place in the last block
        side["pos"][17 + 64 + 4] = side["pos"][17 + 63]
    gate = dict(GATE, skip_distance=np.inf if kind == "all" else 1e-3)
    hip = Hip()
    try:
        s = Session(ctx, hip, 9501, counts, 0, blocks, None, gate=gate, arrays=side)
        for name, lst in (("full", s.full_list), ("every_third", s.full_list[::3]), ("tail", s.full_list[-7:])):
            got = s.run_list(lst)
            n = s.check(lst, got, f"{kind} {name}")
            if kind != "one":
                assert n == (len(lst) if kind == "all" else 0)
        if kind == "one":
            assert n == 1 and got["pairs"][0].tolist() == [17 + 63, 17 + 64 + 4] and got["todo_off"].tolist() == [0, 0, 0, 1]
    finally:
        hip.free_all()


def test_self_lc_per_block(ctx):
    """The time gate follows each block's own flag: enable = 0 appears in the blocks that set self_lc and nowhere else."""
    counts, blocks = (3, 0, 5), [(0, 0, True), (2, 2, False), (0, 2, False), (2, 0, True)]
    hip = Hip()
    try:
        s = Session(ctx, hip, 9600, counts, 16, blocks, [1, 0, 1], gate=dict(GATE, skip_distance=np.inf, desc_thresh=-1.0, lc_time_thresh=300.0))
        for lst in (s.full_list, s.full_list[::2], s.full_list[1::2]):
            got = s.run_list(lst)
            s.check(lst, got, "self_lc")
            off, en = got["todo_off"], got["enable"]
            assert off[-1] == len(lst) and (en[off[1]:off[3]] == 1).all()
        en, t = s.run_list(s.full_list)["enable"], s.arr["time"][:3]     # block 0 whole: every pair is TODO, the time gate is |dt| < 300 s
        assert np.array_equal(en[:9] == 0, (np.abs(t[:, None] - t[None, :]) < 300.0).ravel()) and (en[:9] == 0).sum() >= 3
    finally:
        hip.free_all()


def test_two_runs_agree_and_host_pointers_agree_with_device_pointers(ctx):
    counts, d, blocks = (17, 64, 5), 769, all_pairs(3)
    hip = Hip()
    try:
        for mode in ("radius", "aabb-sim"):
            s = Session(ctx, hip, 9700, counts, d, blocks, [1, 1, 0], mode=mode)
            lst = s.full_list[np.sort(np.random.default_rng(9701).choice(s.total, 1025, replace=False))]
            a, b = s.run_list(lst), s.run_list(lst, shift=1)
            s.check(lst, a, mode)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (mode, k)
            L = len(lst)
            given = dict(pairs=np.full((L, 2), FILL["pairs"], np.int32), T_ref=np.full((L, 4, 4), FILL["T_ref"]), enable=np.full(L, FILL["enable"], np.int32))
            h = ctx.session_gate_list(s.P, *s.tabs[:3], lst, s.arr["pos"], s.arr["T_w"], time=s.arr["time"], desc=s.arr["desc"], pos_gt=s.arr["pos_gt"],
                                      has_gt=s.has_gt, sim_in=s.sim_in, box=s.box, **given)
            for k in OUT + ("todo_off",):
                assert np.asarray(getattr(h, k)).tobytes() == a[k].tobytes(), (mode, k)      # (the untouched capacity included: inout)
    finally:
        hip.free_all()


def test_empty_list_and_empty_session(ctx):
    hip = Hip()
    try:
        for counts, blocks in (((3, 2), []), ((0, 4, 0), [(0, 1, False), (0, 0, True), (1, 2, False)]), ((3, 2), [(0, 1, False)])):
            s = Session(ctx, hip, 9800, counts, 0, blocks, None)
            got = s.run_list(s.full_list[:0])
            assert got["todo_off"].tolist() == [0] * (len(blocks) + 1)
            assert all((got[k] == FILL[k]).all() for k in OUT)
            h = ctx.session_gate_list(s.P, *s.tabs[:3], s.full_list[:0], s.arr["pos"], s.arr["T_w"], time=s.arr["time"])
            assert h.todo_off.tolist() == [0] * (len(blocks) + 1)
    finally:
        hip.free_all()


def test_error_codes(ctx):
    check_error_codes(ctx._lib, ctx._h)
