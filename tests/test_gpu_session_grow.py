"""roman_session_submaps_list_dev / roman_session_submaps_list on the device against roman_session_submaps_dev on the
same device, through the C ABI, and grow_session_pools into submap_align_session_update against build_session_pools into
submap_align_session.

Everything is compared BITWISE.  The outputs lie between guard regions filled with sentinels; their interior starts as
build_session_pools clears its tensors (pool 0.0, src -1, ids -1, descriptors NaN, count and status 0) and is then filled by the FULL
session call — the state of a session between two steps.  A listed slot must then equal, over the whole slot, what the full call
leaves for the new inputs in such buffers; an unlisted slot and every guard must hold what they held; and changed[l] must be the
host's bytewise comparison of the two full builds over slot list[l].  No tolerance anywhere: both sides run the same per-submap
code on the same numbers."""
import subprocess
import sys

import numpy as np
import pytest

import _session_grow as sg
import _session_submaps as sx
from _hipmem import Hip
from test_gpu_session_submaps import make_map
from test_gpu_submaps import FILL, Guarded, sparams

pytestmark = pytest.mark.gpu

CLEAR = dict(pool=0.0, src=-1, ids=-1, desc=sg.NAN_BITS, count=0, status=0)          # what build_session_pools clears its tensors to
CHANGED_FILL = -9


class Session:
    """The tables of a session on the device and its guarded outputs.  interior: CLEAR (a session between two steps) or FILL (sentinels
    everywhere: what an unlisted slot holds beyond its count shows whether it was written)."""

    def __init__(self, ctx, hip, P, maps, d=0, shift=0, interior=CLEAR):
        self.ctx, self.hip, self.P, self.d, self.shift = ctx, hip, P, d, int(shift)
        self.F = maps[0][0].shape[1]
        self.tables(maps)
        S, cap, Fo = int(self.t["sub_off"][-1]), P.cap, P.point_dim + self.F - 3
        self.S, self.rows, self.Fo = S, S * cap, Fo
        self.out = dict(pool=Guarded(hip, self.rows * Fo, np.float64, FILL["pool"], self.shift), count=Guarded(hip, S, np.int32, FILL["count"]),
                        src=Guarded(hip, self.rows, np.int32, FILL["src"]), status=Guarded(hip, S, np.int32, FILL["status"]),
                        ids=Guarded(hip, self.rows, np.int64, FILL["ids"]), desc=Guarded(hip, S * d, np.float64, FILL["desc"]) if d else None)
        if interior is not FILL:
            for k, g in self.out.items():
                if g is not None and g.n:
                    a = np.full(g.n, interior[k], dtype=g.dtype)
                    assert hip.lib.hipMemcpy(g.ptr, a.ctypes.data, a.nbytes, 1) == 0

    def tables(self, maps):
        """(new) tables and centres: the same shapes, other contents"""
        t = self.t = sx.session_of(maps)
        hip = self.hip
        self.N = int(t["seg_off"][-1])
        self.dF = hip.upload(np.concatenate([np.zeros(self.shift), t["feats"].ravel()])) + 8 * self.shift
        self.dT, self.dI = hip.upload(t["times"]), hip.upload(t["ids"])

    def _args(self):
        t, o = self.t, self.out
        return (self.P, self.F, t["seg_off"], self.dF if self.N else None, self.dT if self.N else None, t["sub_off"], t["descs"]), \
            (o["pool"].ptr, o["count"].ptr, o["src"].ptr, o["status"].ptr), \
            dict(seg_ids_ptr=self.dI, ids_out_ptr=o["ids"].ptr, desc_dim=self.d, desc_out_ptr=o["desc"].ptr if self.d else None)

    def full(self):
        a, b, kw = self._args()
        self.ctx.session_submaps_dev(*a, *b, **kw)
        self.ctx.sync()
        return self.get()

    def listed(self, lst, want_changed=True):
        """The list call -> changed (host int32[L], guards checked) or None."""
        a, b, kw = self._args()
        ch = Guarded(self.hip, len(lst), np.int32, CHANGED_FILL) if want_changed else None
        self.ctx.session_submaps_list_dev(*a, lst, *b, changed_ptr=ch.ptr if ch is not None else None, **kw)
        self.ctx.sync()
        return ch.get() if ch is not None else None

    def get(self):
        """-> dict of raw host arrays (get() holds the guard regions to their sentinel)"""
        return {k: (v.get() if v is not None else None) for k, v in self.out.items()}


def slot(P, Fo, d, got, g):
    """Every byte of slot g of a dict of raw arrays."""
    cap = P.cap
    return sg.slot_bytes(cap, g, got["pool"].reshape(-1, Fo), got["count"], got["src"], got["status"], got["ids"], got["desc"].reshape(-1, d) if d else None)


def lists_of(sub_off):
    """empty, single (a submap in the middle), all, first plus last of each robot"""
    S = int(sub_off[-1])
    ends = sorted({int(x) for r in range(len(sub_off) - 1) if sub_off[r + 1] > sub_off[r] for x in (sub_off[r], sub_off[r + 1] - 1)})
    return [[], [S // 2] if S else [], list(range(S)), ends]


def perturbed(maps):
    """The maps with one segment's x moved in every robot that has segments, and the t_hi of every robot's first submap lowered to
    just behind that submap's own time: whatever it held that was first seen later is lost.  A robot's third submap loses its
    whole time window: it becomes EMPTY (every row of its slot is pad, its descriptor NaN)."""
    out = []
    for feats, times, ids, descs in maps:
        feats, descs = feats.copy(), descs.copy()
        if len(feats):
            feats[0, 0] += 0.125
        if len(descs):
            descs[0]["t_hi"] = descs[0]["time"] + 0.5
        if len(descs) >= 3:
            descs[2]["t_hi"] = -np.inf
        out.append((feats, times, ids, descs))
    return out


# (N_r, S_r) per robot: R in {1, 3}; N_r in {0, 1, 63, 64, 65, 257}; S_r in {0, 1, 3}; 63 rows in front, so that with the odd F map 1 starts at 8 mod 16
GRID = [[(257, 3)], [(63, 3), (257, 3), (65, 1)], [(64, 3), (0, 1), (1, 3)], [(65, 1), (257, 0), (63, 3)], [(0, 3), (64, 1), (65, 3)]]
VARIANTS = [(3, 3, 0), (23, 3, 16), (24, 2, 16)]                             # F, point_dim, desc_dim
IDS = ["F3", "F23-odd", "F24-shifted"]


def variant(v):
    F, pd, d = VARIANTS[v]
    P = sparams(pd, max_size=[40, 7, None][v], cap=[None, None, 12][v], by_time=(v == 1), radius=[15.0, None, 20.0][v])
    return F, d, P, [np.inf, 60.0, np.inf][v]


@pytest.mark.parametrize("v", [0, 1, 2], ids=IDS)
def test_the_same_inputs_change_nothing(ctx, v):
    """(a) Behind the full call, every list over the same inputs: every flag 0, every byte as it was."""
    hip = Hip()
    try:
        F, d, P, tt = variant(v)
        for k, shape in enumerate(GRID):
            maps = [make_map(100 * k + 10 * r + v + 1, N, F, S, time_threshold=tt) for r, (N, S) in enumerate(shape)]
            if v == 1 and len(shape) > 1 and shape[0][0] % 2:
                assert (shape[0][0] * F * 8) % 16 == 8
            s = Session(ctx, hip, P, maps, d, shift=int(v == 2))
            was = s.full()
            assert was["count"].max() > 0
            for lst in lists_of(s.t["sub_off"]):
                changed = s.listed(lst)
                assert changed.shape == (len(lst),) and not changed.any(), (shape, lst, changed)
                now = s.get()
                for name in was:
                    assert (was[name] is None) == (now[name] is None) and (was[name] is None or was[name].tobytes() == now[name].tobytes()), (shape, lst, name)
            hip.free_all()
    finally:
        hip.free_all()


@pytest.mark.parametrize("v", [0, 1, 2], ids=IDS)
def test_listed_slots_follow_the_new_inputs_and_unlisted_slots_stay(ctx, v):
    """(b) One segment's x perturbed and one t_hi lowered per robot (a submap loses rows): listed slots equal the fresh full call's,
    pad included; unlisted slots and guards hold what they held; changed is the host's comparison of the two full builds.  The
    first-plus-last list runs once more over sentinel interiors without `changed`: an unlisted slot's sentinels beyond its count
    survive, a listed slot's are cleared."""
    hip = Hip()
    try:
        F, d, P, tt = variant(v)
        shrank = flagged = unflagged = 0
        for k, shape in enumerate(GRID):
            old_maps = [make_map(100 * k + 10 * r + v + 1, N, F, S, time_threshold=tt) for r, (N, S) in enumerate(shape)]
            new_maps = perturbed(old_maps)
            shift = int(v == 2)
            e_old = Session(ctx, hip, P, old_maps, d, shift).full()
            e_new = Session(ctx, hip, P, new_maps, d, shift).full()
            S, Fo = len(e_old["count"]), P.point_dim + F - 3
            differs = np.array([slot(P, Fo, d, e_old, g) != slot(P, Fo, d, e_new, g) for g in range(S)], dtype=bool)
            shrank += int((e_new["count"] < e_old["count"]).sum())
            for lst in lists_of(sx.session_of(old_maps)["sub_off"]):
                s = Session(ctx, hip, P, old_maps, d, shift)
                s.full()
                s.tables(new_maps)
                changed = s.listed(lst)
                got = s.get()
                for g in range(S):
                    want = e_new if g in lst else e_old
                    assert slot(P, Fo, d, got, g) == slot(P, Fo, d, want, g), (shape, lst, g, "listed" if g in lst else "unlisted")
                assert np.array_equal(changed, differs[np.asarray(lst, dtype=np.int64)].astype(np.int32)), (shape, lst, changed, differs)
                flagged += int(changed.sum()); unflagged += int(len(lst) - changed.sum())
            # sentinels in the interior, no flags
            lst = lists_of(sx.session_of(old_maps)["sub_off"])[3]
            s = Session(ctx, hip, P, old_maps, d, shift, interior=FILL)
            raw_old = s.full()
            s.tables(new_maps)
            assert s.listed(lst, want_changed=False) is None
            got = s.get()
            cap = P.cap
            for g in range(S):
                if g not in lst:
                    assert slot(P, Fo, d, got, g) == slot(P, Fo, d, raw_old, g), (shape, g, "an unlisted slot was written")
                    n = int(got["count"][g])
                    assert (got["src"][g * cap + n:(g + 1) * cap] == FILL["src"]).all() and (got["pool"].reshape(-1, Fo)[g * cap + n:(g + 1) * cap] == FILL["pool"]).all()
                else:
                    assert slot(P, Fo, d, got, g) == slot(P, Fo, d, e_new, g), (shape, g, "a listed slot over sentinels")
            hip.free_all()
        assert shrank >= 3, "hardly a submap lost rows: the pad contract was not exercised"
        assert flagged >= 5 and unflagged >= 1, (flagged, unflagged)
    finally:
        hip.free_all()


def test_listed_submaps_beyond_lds_take_their_own_scratch_slices(ctx):
    """(c) One map of 5 000 candidates per submap (no radius, an infinite time window: above the 4096 of LDS) behind a small one, two
    of its three submaps listed: two scratch slices, at 0 and 904, where the full call has three.  Ordered (ranks over LDS and
    scratch) and in map order with truncation."""
    hip = Hip()
    try:
        old_maps = [make_map(22, 65, 3, 1), make_map(21, 5000, 3, 3)]
        new_maps = perturbed(old_maps)
        new_maps[1][3][0]["t_hi"] = new_maps[1][3][2]["t_hi"] = np.inf       # (the big map keeps its 5 000 candidates everywhere)
        T = np.array(new_maps[1][3]["T_center_odom"][2], dtype=np.float64).reshape(4, 4)
        T[0, 3] -= 1.0                                                       # (its last submap looks from one metre further along x: every row changes)
        new_maps[1][3]["T_center_odom"][2] = T.reshape(new_maps[1][3]["T_center_odom"][2].shape)
        for P in (sparams(3, max_size=40), sparams(3, max_size=40, by_time=True), sparams(3, max_size=None, cap=4500)):
            e_old = Session(ctx, hip, P, old_maps).full()
            e_new = Session(ctx, hip, P, new_maps).full()
            s = Session(ctx, hip, P, old_maps)
            s.full()
            s.tables(new_maps)
            lst = [1, 3]
            changed = s.listed(lst)
            got = s.get()
            for g in range(4):
                want = e_new if g in lst else e_old
                assert slot(P, 3, 0, got, g) == slot(P, 3, 0, want, g), (P.max_size, P.cap, g)
            assert changed.tolist() == [int(slot(P, 3, 0, e_old, g) != slot(P, 3, 0, e_new, g)) for g in lst] and changed[1] == 1
            assert got["count"][1] == min(P.cap, 5000) and got["count"][3] == min(P.cap, 5000)
            hip.free_all()
    finally:
        hip.free_all()


def test_the_host_form_gives_the_same_bytes(ctx):
    """(d) roman_session_submaps_list over NumPy arrays against the device-pointer form."""
    hip = Hip()
    try:
        F, d, P, tt = variant(1)
        old_maps = [make_map(31, 257, F, 3, time_threshold=tt), make_map(32, 0, F, 1), make_map(33, 65, F, 2, time_threshold=tt)]
        new_maps = perturbed(old_maps)
        s = Session(ctx, hip, P, old_maps, d)
        was = s.full()
        s.tables(new_maps)
        lst = [0, 3, 5]
        changed = s.listed(lst)
        got = s.get()
        t = sx.session_of(new_maps)
        Fo = P.point_dim + F - 3
        h = {k: (None if a is None else a.copy()) for k, a in was.items()}
        res, ch = ctx.session_submaps_list(P, t["seg_off"], t["feats"], t["times"], t["sub_off"], t["descs"], lst, h["pool"].reshape(-1, Fo), h["count"], h["src"],
                                           h["status"], seg_ids=t["ids"], ids_out=h["ids"], desc_dim=d, desc_out=h["desc"].reshape(-1, d))
        assert np.array_equal(ch, changed) and changed.any()
        for name, a in (("pool", res.pool), ("count", res.count), ("src", res.src), ("status", res.status), ("ids", res.ids), ("desc", res.desc)):
            assert np.ascontiguousarray(a).tobytes() == got[name].tobytes(), name
        # without flags, and an empty list
        res2, none = ctx.session_submaps_list(P, t["seg_off"], t["feats"], t["times"], t["sub_off"], t["descs"], [], res.pool, res.count, res.src, res.status,
                                              seg_ids=t["ids"], ids_out=res.ids, desc_dim=d, desc_out=res.desc, want_changed=False)
        assert none is None and res2.pool.tobytes() == got["pool"].tobytes()
    finally:
        hip.free_all()


def test_error_codes_and_empty_calls_on_a_context(ctx):
    import test_session_grow_abi as abi
    from roman_amd import _abi
    lib = ctx._lib
    abi.check_error_codes(lib, ctx._h)
    for host in (False, True):
        assert abi.Args(lst=()).call(lib, host, ctx._h) == _abi.ROMAN_OK                      # L == 0: nothing is dereferenced
        assert abi.Args(lst=None).call(lib, host, ctx._h) == _abi.ROMAN_OK
        assert abi.Args(lst=(), n=(), s=()).call(lib, host, ctx._h) == _abi.ROMAN_OK          # R == 0


# ---------------------------------------------------------------------------------------------
# (e) end to end: torch holds the device memory, so this runs in a process of its own with torch imported first
# ---------------------------------------------------------------------------------------------
def run_end_to_end():
    import torch
    import _session_update as su
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import SubmapParams, build_session_pools, grow_session_pools
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    D = sg.D
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.65,
                          single_robot_lc=True, single_robot_lc_time_thresh=40.0)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams(max_size=40, radius=15.0, time_threshold=10.0, pruning_method='distance', submap_descriptor='mean_semantic')
    session = sg.GrowingSession(reg, 3, params, steps=3)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    state, align_state, before = None, sa.SessionAlignState(), None
    aligned = kept = 0
    for k in range(3):
        rows = None
        if k == 2:                                                           # a member of an old submap of robot 0 leaves the place
            q = before[0]
            s_ = int(np.nonzero((q.count > 1) & (q.count < q.cap))[0][0])
            row = int(q.src[s_, 0])
            session.edit(0, row, feats=session.full[0].feats[row, :3] + 1000.0)
            rows = [[row], None, None]
        tables, centers = session.stage(k)
        pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device=dev, changed_rows=rows)
        want = build_session_pools(reg, tables, centers, params, ctx=ctx, device=dev)
        for got, w in zip(pools, want):
            sx.same_pool(got, w)
        sx.one_storage(pools, "pool"); sx.one_storage(pools, "ids_dev"); sx.one_storage(pools, "desc_dev")
        assert sa._one_storage(torch, [q.pool for q in pools]).data_ptr() == pools[0].pool.data_ptr()
        if k:
            expect = sg.differing_slots(before, want)
            for r in range(3):
                assert np.array_equal(touched[r], expect[r]), (k, r, touched[r], expect[r])
            kept += int(sum((~t).sum() for t in touched))
        got_lc = sa.submap_align_session_update(align_state, p, pools, touched, None, io, registration=reg)
        want_lc = sa.submap_align_session(p, want, None, io, registration=reg)
        assert list(got_lc) == list(want_lc) == blocks
        for key in blocks:
            su.equal(got_lc[key], want_lc[key])
            aligned += int((want_lc[key].clipper_num_associations >= 4).sum())
        before = want
    assert aligned >= 4, "hardly a pair aligned: the comparison would show nothing"
    assert kept >= 1, "every submap was touched at every step: the flags selected nothing"
    ctx.close()
    print(f"{aligned} pairs aligned, {kept} old submaps left untouched\nSESSION_GROW_OK")


def test_grown_pools_to_loop_closures_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_session_grow as t; t.run_end_to_end()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_GROW_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

