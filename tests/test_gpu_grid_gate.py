"""roman_grid_gate_dev / roman_grid_gate on the device against the NumPy restatement of the contract (tests/_grid_gate_oracle.py),
through the C ABI.

Exact: flags, pairs (content and order), n_todo, enable, NaN patterns.  dist, sim, yaw_deg, T_ij, T_ref: 1e-12 * max(1, |x|) —
dist and T_ij are a few products and sums of values below 1e2 (an ulp of 64 is 1.4e-14); a cosine over d <= 769 terms in another
order differs by at most d * 2^-53 = 8.5e-14; atan2 in degrees carries a few ulps of 180 (2.8e-14 each).  Generated grids carry no
borderline flag (clean_grid raises on a seed that does)."""
import numpy as np
import pytest

import _grid_gate_oracle as go
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import grid_gate_params

pytestmark = pytest.mark.gpu

G = 64                                       # guard elements on either side of every output
FILL = dict(dist=-7.25, flags=-77, yaw_deg=-6.5, sim=-5.5, T_ij=-4.5, pairs=-3, T_ref=-2.5, enable=-9, n_todo=-11)
DTYPE = dict(dist=np.float64, flags=np.int32, yaw_deg=np.float64, sim=np.float64, T_ij=np.float64, pairs=np.int32, T_ref=np.float64,
             enable=np.int32, n_todo=np.int32)
REL = 1e-12


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    inf = ~fin & ~np.isnan(want)
    return bool(np.array_equal(got[inf], want[inf]) and np.all(np.abs(got[fin] - want[fin]) <= REL * np.maximum(1.0, np.abs(want[fin]))))


class Guarded:
    """A device array between two guard regions, everything filled with a sentinel (`shift`: elements the array is moved off its
    natural position: one double leaves a 16-byte boundary)."""

    def __init__(self, hip, n, dtype, fill, shift=0):
        self.hip, self.n, self.dtype, self.fill, self.lead = hip, int(n), np.dtype(dtype), fill, G + shift
        self.base = hip.upload(np.full(self.n + 2 * G + shift, fill, dtype=dtype))
        self.ptr = self.base + self.lead * self.dtype.itemsize

    def get(self):
        whole = self.hip.download(self.base, (self.n + self.lead + G,), self.dtype)
        assert (whole[:self.lead] == self.fill).all() and (whole[self.lead + self.n:] == self.fill).all(), "a guard region was written"
        return whole[self.lead:self.lead + self.n].copy()


def gate_params(d, radius=12.0, skip_distance=np.inf, desc_thresh=0.6, single_robot_lc=True, lc_time_thresh=60.0):
    return dict(radius=radius, skip_distance=skip_distance, desc_thresh=desc_thresh if d else 0.0, single_robot_lc=single_robot_lc,
                lc_time_thresh=lc_time_thresh)


def run_dev(ctx, hip, a, b, gate, shift=0):
    """roman_grid_gate_dev over guarded outputs -> dict of host arrays in the C ABI's shapes (compact arrays at full capacity)."""
    S0, S1 = len(a["pos"]), len(b["pos"])
    d = 0 if a["desc"] is None else a["desc"].shape[1]
    B = S0 * S1

    def up(x):
        if x is None or x.size == 0:
            return None
        return hip.upload(np.concatenate([np.zeros(shift), np.asarray(x, dtype=np.float64).ravel()])) + 8 * shift
    ins = [dict(pos=up(s["pos"]), gt=up(s["pos_gt"]), T_w=up(s["T_w"]), time=up(s["time"]), desc=up(s["desc"]) if d else None) for s in (a, b)]
    size = dict(dist=B, flags=B, yaw_deg=B, sim=B, T_ij=16 * B, pairs=2 * B, T_ref=16 * B, enable=B, n_todo=1)
    out = {k: Guarded(hip, n, DTYPE[k], FILL[k], shift) for k, n in size.items()}
    P = grid_gate_params(desc_dim=d, **gate)
    ctx.grid_gate_dev(P, S0, S1, ins[0]["pos"], ins[0]["T_w"], ins[1]["pos"], ins[1]["T_w"], out["dist"].ptr, out["flags"].ptr, out["yaw_deg"].ptr,
                      out["sim"].ptr, out["T_ij"].ptr, out["pairs"].ptr, out["T_ref"].ptr, out["enable"].ptr, out["n_todo"].ptr,
                      time0_ptr=ins[0]["time"], time1_ptr=ins[1]["time"], desc0_ptr=ins[0]["desc"], desc1_ptr=ins[1]["desc"],
                      pos_gt0_ptr=ins[0]["gt"], pos_gt1_ptr=ins[1]["gt"])
    ctx.sync()
    got = {k: v.get() for k, v in out.items()}
    for k in ("dist", "flags", "yaw_deg", "sim"):
        got[k] = got[k].reshape(S0, S1)
    got["T_ij"] = got["T_ij"].reshape(S0, S1, 4, 4); got["pairs"] = got["pairs"].reshape(B, 2); got["T_ref"] = got["T_ref"].reshape(B, 4, 4)
    return got


def check(o, got, tag=""):
    n = o["n_todo"]
    fin = {k: np.isfinite(o[k]) & np.isfinite(got[k]) for k in ("dist", "sim", "yaw_deg", "T_ij")}
    err = {k: float(np.max(np.abs(got[k][m] - o[k][m]), initial=0.0)) for k, m in fin.items()}
    print(f"{tag}: n_todo={n} of {o['flags'].size} max abs errors {err}")
    assert int(got["n_todo"][0]) == n, tag
    assert np.array_equal(got["flags"], o["flags"]), tag
    assert np.array_equal(got["pairs"][:n], o["pairs"]), tag
    assert np.array_equal(got["enable"][:n], o["enable"]), tag
    for k in ("dist", "sim", "yaw_deg", "T_ij"):
        assert close(got[k], o[k]), (tag, k)
    assert close(got["T_ref"][:n], o["T_ref"]), tag
    assert got["T_ref"][:n].tobytes() == got["T_ij"][o["pairs"][:, 0], o["pairs"][:, 1]].tobytes(), (tag, "T_ref is not the pair's T_ij")
    assert (got["pairs"][n:] == FILL["pairs"]).all() and (got["T_ref"][n:] == FILL["T_ref"]).all() and (got["enable"][n:] == FILL["enable"]).all(), \
        (tag, "capacity slots beyond n_todo were written")


SHAPES = [(0, 3), (3, 0), (1, 1), (3, 5), (17, 64), (65, 63), (40, 40), (130, 129)]
DIMS = [0, 1, 16, 769]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S0,S1", SHAPES)
def test_shapes_against_the_oracle(ctx, S0, S1, d):
    """Every shape x descriptor length; skip_distance finite / infinite, ground truth on neither / one / both sides and the time
    gate alternate over the cases; every second case runs on buffers moved off their 16-byte alignment."""
    v = SHAPES.index((S0, S1)) + DIMS.index(d)
    gate = gate_params(d, skip_distance=[np.inf, 25.0][v % 2], single_robot_lc=bool((v // 2) % 2 == 0))
    a, b = go.clean_grid(7000 + 10 * SHAPES.index((S0, S1)) + DIMS.index(d), S0, S1, d, gt=[(False, False), (True, False), (True, True)][v % 3], **gate)
    hip = Hip()
    try:
        got = run_dev(ctx, hip, a, b, gate, shift=v % 2)
        if S0 == 0 or S1 == 0:
            assert int(got["n_todo"][0]) == 0
            return
        o = go.grid_gate_oracle(a, b, **gate)
        if S0 * S1 >= 1000:
            bits = (go.NEARBY, go.TODO) if (d or np.isfinite(gate["skip_distance"])) else (go.NEARBY,)
            classes = [(o["flags"] & bit) != 0 for bit in bits]
            assert all(0 < c.sum() < c.size for c in classes), "the case does not exercise both sides of a gate"
        check(o, got, f"S0={S0} S1={S1} d={d}")
    finally:
        hip.free_all()


def _two(pa, pb, desc_a=None, desc_b=None):
    side = lambda p, dd: dict(pos=np.array(p, dtype=np.float64).reshape(-1, 3), pos_gt=None, time=np.zeros(len(p)),
                              T_w=np.stack([go.yaw_pose(0.25 * k, q) for k, q in enumerate(p)]), desc=None if dd is None else np.array(dd, dtype=np.float64))
    return side(pa, desc_a), side(pb, desc_b)


def test_exact_ties_fall_on_the_side_the_contract_names(ctx):
    hip = Hip()
    try:
        a, b = _two([(0.0, 0.0, 0.0)], [(6.0, 8.0, 0.0)])                      # dist is exactly 10
        got = run_dev(ctx, hip, a, b, gate_params(0, radius=5.0, skip_distance=10.0))
        assert got["dist"][0, 0] == 10.0
        assert got["flags"][0, 0] == go.TODO, "dist == 2 * radius is not nearby; dist == skip_distance is not skipped"
        assert np.isnan(got["yaw_deg"][0, 0]) and np.isposinf(got["sim"][0, 0]) and got["n_todo"][0] == 1
        got = run_dev(ctx, hip, a, b, gate_params(0, radius=np.nextafter(5.0, 6.0), skip_distance=np.nextafter(10.0, 0.0)))
        assert got["flags"][0, 0] == (go.NEARBY | go.SKIP) and got["n_todo"][0] == 0 and got["yaw_deg"][0, 0] == np.abs(np.rad2deg(0.0))
        # cosine exactly 0.5 at the threshold 0.5: not gated; an all-zero descriptor: similarity 0, gated
        a, b = _two([(0.0, 0.0, 0.0)] * 2, [(1.0, 0.0, 0.0)] * 2, [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]], [[1.0, 0.0, 0.0, 0.0], [0.0, 3.0, 0.0, 0.0]])
        got = run_dev(ctx, hip, a, b, gate_params(4, radius=5.0, desc_thresh=0.5))
        assert got["sim"].tolist() == [[0.5, 0.5], [0.0, 0.0]]
        assert got["flags"].tolist() == [[go.NEARBY | go.TODO] * 2, [go.NEARBY | go.GATED] * 2]
        assert got["pairs"][:2].tolist() == [[0, 0], [0, 1]] and got["n_todo"][0] == 2
    finally:
        hip.free_all()


def test_all_none_and_one_pair_todo(ctx):
    hip = Hip()
    try:
        S0, S1 = 33, 70                                                          # 2310 pairs: several per thread in the scan
        gate = gate_params(16, skip_distance=np.inf, desc_thresh=-2.0)
        a, b = go.clean_grid(11, S0, S1, 16, **gate)
        o = go.grid_gate_oracle(a, b, **gate)
        got = run_dev(ctx, hip, a, b, gate)
        assert o["n_todo"] == S0 * S1 and np.array_equal(got["pairs"], np.stack(np.divmod(np.arange(S0 * S1), S1), axis=1))
        check(o, got, "all todo")
        gate = gate_params(16, skip_distance=-1.0)
        got = run_dev(ctx, hip, a, b, gate)
        o = go.grid_gate_oracle(a, b, **gate)
        assert o["n_todo"] == 0 and ((got["flags"] & go.SKIP) != 0).all()
        check(o, got, "none todo")
        a["pos"][:] = 0.0; a["pos"][-1] = (100.0, 0.0, 0.0); b["pos"][:] = (200.0, 0.0, 0.0); b["pos"][-1] = (100.0, 0.0, 1.0)
        gate = gate_params(16, skip_distance=5.0, desc_thresh=-2.0)
        assert not go.borderline(a, b, **gate)
        o = go.grid_gate_oracle(a, b, **gate)
        got = run_dev(ctx, hip, a, b, gate)
        assert o["pairs"].tolist() == [[S0 - 1, S1 - 1]]
        check(o, got, "one todo, last cell")
    finally:
        hip.free_all()


def test_two_runs_agree_bit_for_bit_and_the_host_pointer_call_gives_the_same_bytes(ctx):
    hip = Hip()
    try:
        gate = gate_params(769, skip_distance=30.0)
        a, b = go.clean_grid(21, 37, 41, 769, gt=(True, True), **gate)
        r1 = run_dev(ctx, hip, a, b, gate)
        r2 = run_dev(ctx, hip, a, b, gate, shift=1)
        for k in r1:
            assert r1[k].tobytes() == r2[k].tobytes(), f"{k} differs between two calls"
        B = 37 * 41
        res = ctx.grid_gate(grid_gate_params(desc_dim=769, **gate), a["pos"], a["T_w"], b["pos"], b["T_w"], time0=a["time"], time1=b["time"],
                            desc0=a["desc"], desc1=b["desc"], pos_gt0=a["pos_gt"], pos_gt1=b["pos_gt"],
                            pairs=np.full((B, 2), FILL["pairs"], np.int32), T_ref=np.full((B, 4, 4), FILL["T_ref"]), enable=np.full(B, FILL["enable"], np.int32))
        assert res.n_todo == int(r1["n_todo"][0]) and 0 < res.n_todo < B
        for k in ("dist", "flags", "yaw_deg", "sim", "T_ij", "pairs", "T_ref", "enable"):
            assert getattr(res, k).tobytes() == r1[k].tobytes(), f"{k}: host-pointer call differs from the device-pointer call"
        check(go.grid_gate_oracle(a, b, **gate), r1, "769-d, ground truth on both sides")
    finally:
        hip.free_all()


def sides_case(gt, seed=9112):
    """A 2 x 5 grid (a row spans two waves of GRID_TJ = 4 columns) on which every per-side array differs between the sides: 3-d
    descriptors, distinct times under the time gate, boxes, a given similarity.  gt (True, True): the distances come from pos_gt
    and pos is not read; (True, False): they come from pos, and side 0's pos_gt must not be used."""
    gate = gate_params(3, skip_distance=35.0)
    a, b = go.clean_grid(seed, 2, 5, 3, gt=gt, **gate)
    rng = np.random.default_rng(seed + 1)
    boxes = [np.hstack([s["pos"] - rng.uniform(5.0, 25.0, (len(s["pos"]), 3)), s["pos"] + rng.uniform(5.0, 25.0, (len(s["pos"]), 3))]) for s in (a, b)]
    return a, b, boxes, rng.uniform(0.2, 0.95, (2, 5)), gate


def sides_oracle(a, b, boxes, sim_in, gate, aabb, given):
    """The NumPy restatement of the entry that serves (aabb, given)."""
    import _fill_boxes_oracle as fo
    rest = {k: v for k, v in gate.items() if k != "radius"}
    if not given:
        return fo.aabb_gate_oracle(a, b, *boxes, **rest) if aabb else go.grid_gate_oracle(a, b, **gate)
    o = fo.aabb_gate_oracle(a, b, *boxes, sim_in=sim_in, **rest)
    if not aabb:                                 # the classes of a given similarity as the box oracle derives them; NEARBY and the yaw by the radius
        r = go.grid_gate_oracle({**a, "desc": None}, {**b, "desc": None}, **gate)
        o["flags"] = (o["flags"] & ~go.NEARBY) | (r["flags"] & go.NEARBY); o["yaw_deg"] = r["yaw_deg"]
    return o


@pytest.mark.parametrize("gt", [(True, True), (True, False)], ids=["gt-both", "gt-one"])
@pytest.mark.parametrize("entry", ["grid_gate", "grid_gate_sim", "grid_gate_aabb", "grid_gate_aabb-sim_in"])
def test_every_entry_keeps_its_two_sides_apart(ctx, entry, gt):
    """Each of the six entry points, host and `_dev`, against the oracle on sides_case(): an entry that hands the gate side 1's
    pos, pos_gt, T_w, time, desc or box for side 0's, sim for sim_in or T_ref for T_ij misses it."""
    aabb, given = "aabb" in entry, "sim" in entry
    a, b, boxes, sim_in, gate = sides_case(gt)
    d = 0 if given else 3
    P = grid_gate_params(None if aabb else gate["radius"], desc_dim=d, **{k: v for k, v in gate.items() if k != "radius"})
    o = sides_oracle(a, b, boxes, sim_in, gate, aabb, given)
    assert 0 < o["n_todo"] < 10 and set(o["enable"].tolist()) == {0, 1} and 0 < ((o["flags"] & go.NEARBY) != 0).sum() < 10, "the case lost its classes"
    hip = Hip()
    try:
        up = lambda x: None if x is None else hip.upload(np.asarray(x, dtype=np.float64).ravel())
        size = dict(dist=10, flags=10, yaw_deg=10, sim=10, T_ij=160, pairs=20, T_ref=160, enable=10, n_todo=1)
        out = {k: Guarded(hip, n, DTYPE[k], FILL[k]) for k, n in size.items()}
        handed = dict(pairs=np.full((10, 2), FILL["pairs"], np.int32), T_ref=np.full((10, 4, 4), FILL["T_ref"]), enable=np.full(10, FILL["enable"], np.int32))
        pos = (a["pos"], a["T_w"], b["pos"], b["T_w"])
        kw = dict(time0=a["time"], time1=b["time"], pos_gt0=a["pos_gt"], pos_gt1=b["pos_gt"])
        if not given:
            kw.update(desc0=a["desc"], desc1=b["desc"])
        dev = [up(x) for x in pos] + [out[k].ptr for k in size]
        dkw = {k + "_ptr": up(v) for k, v in kw.items()}
        if entry == "grid_gate_sim":                           # the similarity travels in the sim slot and comes back as it went
            dev[7] = up(sim_in)
            h = ctx.grid_gate_sim(P, sim_in, *pos, **kw, **handed)
            ctx.grid_gate_sim_dev(P, 2, 5, *dev, **dkw)
        elif aabb:
            h = ctx.grid_gate_aabb(P, boxes[0], boxes[1], *pos, **kw, sim_in=sim_in if given else None, **handed)
            ctx.grid_gate_aabb_dev(P, 2, 5, *dev, **dkw, box0_ptr=up(boxes[0]), box1_ptr=up(boxes[1]), sim_in_ptr=up(sim_in) if given else None)
        else:
            h = ctx.grid_gate(P, *pos, **kw, **handed)
            ctx.grid_gate_dev(P, 2, 5, *dev, **dkw)
        ctx.sync()
        got = {k: v.get() for k, v in out.items()}
        if given:                                              # an entry that is given the similarity does not write one
            assert (got["sim"] == FILL["sim"]).all()
            got["sim"] = hip.download(dev[7], (10,), np.float64) if entry == "grid_gate_sim" else sim_in.ravel()
        for k in ("dist", "flags", "yaw_deg", "sim"):
            got[k] = got[k].reshape(2, 5)
        got["T_ij"] = got["T_ij"].reshape(2, 5, 4, 4); got["pairs"] = got["pairs"].reshape(10, 2); got["T_ref"] = got["T_ref"].reshape(10, 4, 4)
        check(o, got, f"{entry}_dev {gt}")
        host = {k: getattr(h, k) for k in size if k != "n_todo"}
        host["n_todo"] = np.array([h.n_todo])
        check(o, host, f"{entry} {gt}")
    finally:
        hip.free_all()


def test_error_codes(ctx):
    gate = gate_params(4)
    a, b = go.clean_grid(5, 3, 4, 4, **gate)
    call = lambda P, aa=a, bb=b: ctx.grid_gate(P, aa["pos"], aa["T_w"], bb["pos"], bb["T_w"], time0=aa["time"], time1=bb["time"], desc0=aa["desc"], desc1=bb["desc"])
    ok = grid_gate_params(desc_dim=4, **gate)
    assert call(ok).n_todo > 0
    bad = []
    P = grid_gate_params(desc_dim=4, **{**gate, "radius": np.nan}); bad.append((P, _abi.ROMAN_E_INVALID))
    P = grid_gate_params(desc_dim=-1, **gate); bad.append((P, _abi.ROMAN_E_INVALID))
    P = grid_gate_params(desc_dim=4, **gate); P.reserved0 = 1; bad.append((P, _abi.ROMAN_E_INVALID))
    P = grid_gate_params(desc_dim=4, **gate); P.reserved[1] = 1; bad.append((P, _abi.ROMAN_E_INVALID))
    P = grid_gate_params(desc_dim=4, **{**gate, "radius": -1.0}); bad.append((P, _abi.ROMAN_E_UNSUPPORTED))
    P = grid_gate_params(desc_dim=4, **{**gate, "radius": None}); bad.append((P, _abi.ROMAN_E_UNSUPPORTED))
    for P, code in bad:
        with pytest.raises(_abi.RomanHipError) as e:
            call(P)
        assert e.value.code == code
    with pytest.raises(_abi.RomanHipError) as e:                                   # desc NULL with desc_dim > 0
        call(ok, {**a, "desc": None}, b)
    assert e.value.code == _abi.ROMAN_E_INVALID
    empty = {k: (None if v is None else v[:0]) for k, v in a.items()}
    assert call(ok, empty, b).n_todo == 0 and call(ok, a, {k: (None if v is None else v[:0]) for k, v in b.items()}).n_todo == 0
    assert call(grid_gate_params(desc_dim=4, **{**gate, "skip_distance": np.inf})).n_todo > 0      # +inf is legal
    assert call(ok).n_todo > 0                                                     # the context stays usable
