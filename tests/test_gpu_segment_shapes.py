"""Segment tables from point clouds through the C ABI: roman_segment_shapes* against tests/_segment_shapes_oracle.py.

THE TOLERANCE is derived from the kernel's summation order, not from what the kernel gives.  A sum over the n points of a segment
is a tree of depth D = ceil(n / (64 NW)) - 1 + 6 + (NW - 1): thread t of the team of NW waves (1 below ROMAN_SEG_BLOCK_MIN points,
4 from there on) adds its points one after the other, wave_sum63 adds six levels, the waves' sums are added in wave order.  Hence
  mean         |dm| <= (D + 1) 2^-53 sum|x| / n                       (the + 1: the division)
  covariance   |dC_ij| <= (D + 4) 2^-53 sum|d_i d_j| / n              (the + 4: two subtractions, the product, the division), so
               ||dC||_F <= (D + 4) 2^-53 trace(C)
  eigenvalues  |de_k| <= ||dC||_F + c 2^-53 e0,  c = 64: at most 6 Jacobi sweeps x 3 rotations x 3 roundings, and the oracle's eigh
  ratios       each is an error relative to e0: <= 3 |de| / e0
  extent       8 roundings of a projection plus the turn of the eigenframe, sin <= 2 |de| / gap (Davis-Kahan), times the cloud's
               radius at both ends of a side; volume: the sum of the three relative errors
(`_segment_shapes_oracle.bounds`).  The worst observed deviation over these clouds, as a fraction of its bound, is printed by
test_mixed_list and recorded in profiles/segment_shapes/README.md.

BIT FOR BIT for the bottom_middle centre means the IEEE bits of np.median (x, y) and np.min (z).  A median that is a zero is +0.0
on both sides (np.median ends in a mean, a sum that starts from +0.0).  One case is outside bit equality: the MINIMUM of a cloud that
holds zeros of both signs, where np.min returns whichever it met first (-0.0 == +0.0 to its comparisons) while the device orders
-0.0 below +0.0; there both must be zeros (`same_bits`)."""
import ctypes as C

import numpy as np
import pytest

import _segment_shapes_oracle as so
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import segment_shape_params

pytestmark = pytest.mark.gpu

T = _abi.ROMAN_SEG_BLOCK_MIN
SIZES = [0, 1, 2, 4, 5, 10, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 3 * T + 37]     # the last: several passes of the workgroup path
GUARD = -7.25e300
SIDES = (0.3, 1.1, 2.7)      # eigenvalues s^2 / 12 of a filled box: gaps (e0 - e1) / e0 = 0.83, (e1 - e2) / e0 = 0.15, both >= 0.1


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def cloud(rng, n, shift=(31.0, -17.0, 2.5)):
    """n points uniform in a box of SIDES, turned by a generic rotation and shifted."""
    return (rng.uniform(-0.5, 0.5, (n, 3)) * SIDES) @ rotation(rng).T + np.asarray(shift)


def pack(clouds):
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    if clouds:
        off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.vstack([np.zeros((0, 3))] + [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]))
    return pts, off


FULL = dict(out_stride=10, col_center=0, col_pca=3, col_volume=6, col_extent=7)


def run(ctx, clouds, center_ref="mean", **cols):
    pts, off = pack(clouds)
    P = segment_shape_params(center_ref, **(cols or FULL))
    out = np.full((len(clouds), P.out_stride), GUARD)
    return ctx.segment_shapes(pts, off, P, out=out)


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | ((got == 0.0) & (want == 0.0))))


def check_row(row, st, pts, worst):
    """One FULL row against the oracle within the derived bounds; `worst` collects observed / bound."""
    n = len(pts)
    o = so.segment(pts)
    want_st = (_abi.ROMAN_SEG_EMPTY if n == 0 else 0) | (_abi.ROMAN_SEG_FEW_POINTS if n <= 4 else 0) | \
              (_abi.ROMAN_SEG_DEGENERATE if n > 0 and o["eig"][0] == 0 else 0)
    assert st == want_st, (n, st, want_st)
    if n == 0:
        assert np.array_equal(row, np.zeros(10))
        return
    b = so.bounds(pts, T)
    dc = np.abs(row[:3] - o["center"])
    assert np.all(dc <= b["center"]), (n, dc, b["center"])
    worst["center"] = max(worst.get("center", 0.0), float(np.max(dc / b["center"])))
    if o["eig"][0] == 0:
        assert np.all(np.isnan(row[3:6]))
    else:
        dr = np.abs(row[3:6] - o["ratios"])
        assert np.all(dr <= b["ratio"]), (n, dr, b["ratio"])
        worst["ratio"] = max(worst.get("ratio", 0.0), float(np.max(dr) / b["ratio"]))
    if n <= 4:
        assert np.array_equal(row[6:10], np.zeros(4))
    elif np.isfinite(b["extent"]):
        de = np.abs(row[7:10] - o["extent"])
        assert np.all(de <= b["extent"]), (n, de, b["extent"])
        assert abs(row[6] - o["volume"]) <= b["volume"], (n, row[6], o["volume"], b["volume"])
        assert np.all(np.diff(row[7:10]) >= 0)
        worst["extent"] = max(worst.get("extent", 0.0), float(np.max(de) / b["extent"]))


@pytest.mark.parametrize("N", [0, 1, 3, 67])
def test_mixed_list(ctx, N):
    rng = np.random.default_rng(100 + N)
    sizes = {0: [], 1: [T + 1], 3: [65, 0, T]}.get(N) or [SIZES[i % len(SIZES)] for i in rng.permutation(N)]
    clouds = [cloud(rng, n) for n in sizes]
    out, st = run(ctx, clouds)
    assert out.shape == (N, 10) and st.shape == (N,)
    worst = {}
    for i, c in enumerate(clouds):
        check_row(out[i], int(st[i]), c, worst)
    print(f"N={N}: worst observed / bound = {worst}")
    if N == 67:
        assert set(sizes) == set(SIZES)                          # every size of the list, both paths, in one call


def median_clouds():
    rng = np.random.default_rng(7)
    base = rng.normal(size=(T + 37, 3)) * 3.0
    asc = np.sort(base, axis=0)
    one = np.float64(1.0)
    lastbit = np.stack([np.nextafter(one, 2.0, dtype=np.float64) if i % 2 else one for i in range(10)])
    cases = {
        "odd": base[:65], "even": base[:64], "odd-long": base[:T + 37], "even-long": base[:T + 36], "two": base[:2], "one": base[:1],
        "all-equal": np.tile(base[3], (12, 1)),
        "ties-straddle": np.array([[1.0, 5.0, 0.0]] * 3 + [[2.0, 5.0, 0.0]] * 4 + [[3.0, 6.0, 1.0]] * 3),   # the two middle values tie (x) / differ (y: 5, 5)
        "negative": -np.abs(base[:40]) - 1.0,
        "zeros-same-sign": np.array([[-3.0, -0.0, 1.0], [-0.0, -0.0, -0.0], [-0.0, -0.0, 2.0], [4.0, 5.0, 3.0], [-5.0, -6.0, 4.0]]),
        "zeros-mixed": np.array([[-1.0, 0.0, -0.0], [-0.0, -2.0, 0.0], [0.0, -0.0, 1.0], [2.0, 3.0, 0.0], [-3.0, 0.0, 5.0], [0.0, -0.0, 2.0]]),
        "zeros-mixed-not-selected": np.array([[-0.0, 1.0, 1.0], [0.0, 2.0, 2.0], [3.0, 4.0, 3.0], [4.0, 5.0, 4.0], [5.0, 6.0, 5.0]]),
        "last-bit": np.stack([lastbit, lastbit[::-1], lastbit], axis=1),
        "ascending": asc, "descending": asc[::-1].copy(), "shuffled": asc[rng.permutation(len(asc))],
    }
    return cases


def test_bottom_middle_is_exact(ctx):
    cases = median_clouds()
    names = list(cases)
    out, st = run(ctx, [cases[k] for k in names], center_ref="bottom_middle")
    for i, k in enumerate(names):
        p = cases[k]
        want = np.median(p, axis=0); want[2] = np.min(p[:, 2])
        assert same_bits(out[i, :3], want), (k, out[i, :3], want)
        assert np.array_equal(out[i, :2].view(np.uint64), want[:2].view(np.uint64)), k
        if k != "zeros-mixed":
            assert out[i, 2:3].view(np.uint64)[0] == want[2:3].view(np.uint64)[0], k
        else:                                                    # zeros of both signs are the smallest z: the device's pick is -0.0, its documented order
            assert out[i, 2] == 0.0 and np.signbit(out[i, 2]), out[i, 2]
    # the covariance is taken about the MEAN whichever centre is asked for
    out_m, _ = run(ctx, [cases[k] for k in names])
    assert np.array_equal(out[:, 3:].view(np.uint64), out_m[:, 3:].view(np.uint64))


def test_far_from_the_origin(ctx):
    rng = np.random.default_rng(3)
    for n in (200, T + 100):
        c = (rng.uniform(-0.5, 0.5, (n, 3)) * (0.2, 0.12, 0.05)) @ rotation(rng).T + (8000.0, -6000.0, 40.0)      # a 0.2 m cloud
        out, st = run(ctx, [c])
        check_row(out[0], int(st[0]), c, {})


def planted(rng, m):
    """8 (m + 1) points symmetric under the three mirror planes of a box of SIDES, its eight corners among them, turned and shifted: the
    covariance is diagonal in the box frame, with eigenvalue gaps of at least 0.1 e0 (asserted)."""
    q = rng.uniform(0.0, 0.5, (m, 3)) * SIDES
    q = np.vstack([q, 0.5 * np.asarray(SIDES)[None, :]])
    signs = np.array([[a, b, c] for a in (1, -1) for b in (1, -1) for c in (1, -1)], dtype=np.float64)
    box = (q[:, None, :] * signs[None, :, :]).reshape(-1, 3)
    return box @ rotation(rng).T + (12.0, 7.0, -3.0)


def test_planted_boxes(ctx):
    rng = np.random.default_rng(5)
    clouds = [planted(rng, m) for m in (1, 7, 40, 100)]          # 16, 64, 328, 808 points: both paths
    out, st = run(ctx, clouds)
    for i, c in enumerate(clouds):
        o = so.segment(c)
        assert min(o["eig"][0] - o["eig"][1], o["eig"][1] - o["eig"][2]) >= 0.1 * o["eig"][0]
        b = so.bounds(c, T)
        assert np.all(np.abs(out[i, 7:10] - np.asarray(SIDES)) <= b["extent"]), (out[i, 7:10], b["extent"])
        assert abs(out[i, 6] - np.prod(SIDES)) <= b["volume"]
        assert st[i] == 0


def test_degenerate_clouds(ctx):
    rng = np.random.default_rng(9)
    p = np.array([3.1, -2.7, 0.9])
    t = rng.uniform(-1.0, 1.0, 50)
    line = p + np.outer(t, [1.0, 2.0, -0.5])
    u, v = np.array([1.0, 0.5, 0.25]), np.array([-0.5, 1.0, 0.0])
    plane = p + np.outer(rng.uniform(-1, 1, 80), u) + np.outer(rng.uniform(-0.3, 0.3, 80), v)
    clouds = [p[None, :], np.tile(p, (7, 1)), np.tile(p, (T + 5, 1)), line, plane, cloud(rng, 3), cloud(rng, 4), np.zeros((0, 3))]
    out, st = run(ctx, clouds)
    for i in (0, 1, 2):                                          # one point / all points equal
        assert np.all(np.isnan(out[i, 3:6])) and st[i] & _abi.ROMAN_SEG_DEGENERATE
        assert np.array_equal(out[i, 6:10], np.zeros(4)) and np.array_equal(out[i, :3], p)
    bl, bp = so.bounds(line, T), so.bounds(plane, T)
    assert abs(out[3, 3] - 1.0) <= bl["ratio"] and abs(out[3, 4]) <= bl["ratio"] and abs(out[3, 5]) <= bl["ratio"]
    assert abs(out[4, 5]) <= bp["ratio"]
    for i in (5, 6):                                             # n <= 4
        assert np.array_equal(out[i, 6:10], np.zeros(4)) and st[i] == _abi.ROMAN_SEG_FEW_POINTS
    assert np.array_equal(out[7], np.zeros(10)) and st[7] & _abi.ROMAN_SEG_EMPTY


COLUMN_MAPS = {          # each registration's map into a table of stride 3 + 7 + 16
    "roman": dict(col_center=0, col_pca=3, col_volume=6, col_extent=7),
    "pcavol": dict(col_center=0, col_pca=3, col_volume=6, col_extent=-1),
    "extentvol": dict(col_center=0, col_pca=-1, col_volume=3, col_extent=4),
    "prune-on-device": dict(col_center=0, col_volume=3, col_pca=4, col_extent=-1),
    "centres": dict(col_center=0, col_pca=-1, col_volume=-1, col_extent=-1),
    "no-pca": dict(col_center=5, col_pca=-1, col_volume=0, col_extent=1),
    "no-volume": dict(col_center=20, col_pca=2, col_volume=-1, col_extent=8),
    "no-extent": dict(col_center=9, col_pca=23, col_volume=1, col_extent=-1),
}


@pytest.mark.parametrize("name", list(COLUMN_MAPS))
def test_placement(ctx, name):
    cols = COLUMN_MAPS[name]
    rng = np.random.default_rng(2)
    clouds = [cloud(rng, n) for n in (9, 70, T + 3, 0)]
    ref, _ = run(ctx, clouds)
    pts, off = pack(clouds)
    P = segment_shape_params("mean", 26, **cols)
    # through the _dev entry, on a DEVICE table two rows longer than N: what the kernels leave alone is what is checked (the
    # host-pointer entry mirrors N rows only, so its caller's extra rows could not show a stray store)
    hip = Hip()
    try:
        d_table = hip.upload(np.full((len(clouds) + 2, 26), GUARD)); d_st = hip.upload(np.full(len(clouds) + 2, -1, dtype=np.int32))
        ctx.segment_shapes_dev(hip.upload(pts), hip.upload(off), off, P, d_table, d_st)
        ctx.sync()
        table = hip.download(d_table, (len(clouds) + 2, 26), np.float64); st = hip.download(d_st, (len(clouds) + 2,), np.int32)
    finally:
        hip.free_all()
    assert np.all(st[len(clouds):] == -1) and np.all(st[:len(clouds)] >= 0)
    written = np.zeros(26, dtype=bool)
    for key, w, src in (("col_center", 3, 0), ("col_pca", 3, 3), ("col_volume", 1, 6), ("col_extent", 3, 7)):
        c0 = cols[key]
        if c0 >= 0:
            written[c0:c0 + w] = True
            assert np.array_equal(table[:len(clouds), c0:c0 + w].view(np.uint64), ref[:, src:src + w].view(np.uint64)), key
    assert np.all(table[:len(clouds), ~written] == GUARD) and np.all(table[len(clouds):] == GUARD)


def test_determinism_and_position_independence(ctx):
    rng = np.random.default_rng(21)
    clouds = [cloud(rng, n) for n in (T + 200, 33, 0, 64, T, 7, 2 * T + 1, 129)]
    for ref in ("mean", "bottom_middle"):
        a, sa = run(ctx, clouds, ref)
        b, sb = run(ctx, clouds, ref)
        assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
        perm = rng.permutation(len(clouds))
        c, sc = run(ctx, [clouds[i] for i in perm], ref)
        assert np.array_equal(c.view(np.uint64), a[perm].view(np.uint64)) and np.array_equal(sc, sa[perm])
        for i in (0, 1, 4):                                      # alone: the same bytes as in the middle of the list
            d, sd = run(ctx, [clouds[i]], ref)
            assert d.tobytes() == a[i:i + 1].tobytes() and sd[0] == sa[i]


def test_host_and_device_entries_agree(ctx):
    rng = np.random.default_rng(4)
    clouds = [cloud(rng, n) for n in (5, T + 9, 0, 90)]
    pts, off = pack(clouds)
    P = segment_shape_params("bottom_middle", **FULL)
    host, st_h = run(ctx, clouds, "bottom_middle")
    hip = Hip()
    try:
        d_out = hip.upload(np.full((len(clouds), 10), GUARD)); d_st = hip.upload(np.zeros(len(clouds), dtype=np.int32))
        ctx.segment_shapes_dev(hip.upload(pts), hip.upload(off), off, P, d_out, d_st)
        ctx.sync()
        assert hip.download(d_out, (len(clouds), 10), np.float64).tobytes() == host.tobytes()
        assert np.array_equal(hip.download(d_st, (len(clouds),), np.int32), st_h)
    finally:
        hip.free_all()


def test_guards_leave_the_outputs_untouched(ctx):
    lib = ctx._lib
    rng = np.random.default_rng(1)
    pts, off = pack([cloud(rng, 6), cloud(rng, 9)])
    out = np.full((2, 10), GUARD); st = np.full(2, -5, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    good = segment_shape_params("mean", **FULL)

    def call(P=good, points=vp(pts), seg_off=off, N=2, o=vp(out), s=vp(st), h=ctx._h):
        return lib.roman_segment_shapes(h, points, None if seg_off is None else vp(seg_off), N, None if P is None else C.byref(P), o, s)

    def block(**kw):
        P = segment_shape_params("mean", **{**FULL, **{k: v for k, v in kw.items() if k != "reserved" and k != "center_ref"}})
        if "center_ref" in kw:
            P.center_ref = kw["center_ref"]
        if "reserved" in kw:
            P.reserved[1] = kw["reserved"]
        return P

    bad = [dict(h=None), dict(P=None), dict(seg_off=None), dict(N=-1), dict(seg_off=off + 1), dict(seg_off=np.array([0, 9, 6], dtype=np.int64)),
           dict(P=block(center_ref=2)), dict(P=block(col_pca=-2)), dict(P=block(col_extent=8)), dict(P=block(col_center=8)),
           dict(P=block(col_volume=4)), dict(P=block(col_pca=1)), dict(P=block(reserved=1)), dict(P=block(out_stride=0)), dict(points=None),
           dict(o=None), dict(s=None)]
    for kw in bad:
        assert call(**kw) == _abi.ROMAN_E_INVALID, kw
        assert lib.roman_last_error(kw.get("h", ctx._h))
        assert np.all(out == GUARD) and np.all(st == -5), kw
    hip = Hip()
    try:
        d_out = hip.upload(out); d_st = hip.upload(st); d_pts = hip.upload(pts); d_off = hip.upload(off)
        for kw in (dict(seg_off_dev=None), dict(seg_off_host=None), dict(seg_off_host=np.array([0, 9, 6], dtype=np.int64)), dict(P=block(col_pca=1))):
            rc = lib.roman_segment_shapes_dev(ctx._h, C.c_void_p(d_pts), C.c_void_p(d_off) if "seg_off_dev" not in kw else None,
                                              None if kw.get("seg_off_host", off) is None else vp(kw.get("seg_off_host", off)), 2,
                                              C.byref(kw.get("P", good)), C.c_void_p(d_out), C.c_void_p(d_st))
            assert rc == _abi.ROMAN_E_INVALID, kw
        ctx.sync()
        assert np.all(hip.download(d_out, (2, 10), np.float64) == GUARD) and np.all(hip.download(d_st, (2,), np.int32) == -5)
    finally:
        hip.free_all()
    assert call(N=0, seg_off=np.zeros(1, dtype=np.int64), points=None, o=None, s=None) == _abi.ROMAN_OK
    assert call() == _abi.ROMAN_OK and not np.any(out == GUARD)
