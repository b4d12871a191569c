"""roman_session_frame_select_list_dev / roman_session_frame_select_list on the device against roman_frame_select run
per robot on the same device, through the C ABI.

Everything is compared BITWISE: both sides run the same per-submap code on the same numbers.  The session's outputs start filled with
sentinels; a listed slot must then hold what the per-robot call gives for it — its mask row over all `mask_words` words, zero
beyond the robot's ceil(Nf / 64), with mask_words W and W + 2 —, an unlisted slot must hold its sentinels, and changed[l] must say whether a mask word, the count or 64 bits
of a mean column differ from what the slot held (NaN compared by its bits)."""
import numpy as np
import pytest

from _hipmem import Hip
from roman_amd.runtime import frame_select_params, session_frame_robots
from test_gpu_submaps import Guarded

pytestmark = pytest.mark.gpu

CAP, NSEG = 4, 12
# (Nf, S) per robot: Nf in {0, 1, 64, 65, 130} and S in {0, 1, 5}, every Nf with a robot that holds submaps
SESSIONS = [[(0, 1), (1, 5), (64, 0), (65, 5), (130, 1)], [(130, 5), (0, 0), (65, 1), (64, 5), (1, 1), (0, 5)]]
SENT = dict(mask=np.uint64(0xA5A5A5A5A5A5A5A5), n_sel=np.int32(-7), span=-5.5, mean=-6.25)
THIN = [("all", None, False), ("thin0", 0.0, False), ("thin", 2.5, False), ("one-place", 1.0, True)]


def session(shape, d, extra, seed, one_place=False):
    """The tables of a session: per robot NSEG segment rows, S slots of CAP rows (the third of five EMPTY: count 0), Nf frames with
    UNSORTED times, 1 m apart along a line (or all at one position)."""
    rng = np.random.default_rng(seed)
    n_sub, n_frames = [s for _, s in shape], [nf for nf, _ in shape]
    R, S, NF = len(shape), sum(n_sub), sum(n_frames)
    seg = np.zeros((R * NSEG, 2))
    first = np.floor(rng.uniform(0.0, 1200.0, R * NSEG)) + 0.25
    seg[:, 0], seg[:, 1] = first, first + np.floor(rng.uniform(50.0, 600.0, R * NSEG)) + 0.5
    count = rng.integers(1, CAP + 1, S).astype(np.int32)
    src = np.full((S, CAP), -1, dtype=np.int32)
    ft, fp = np.zeros(NF), np.zeros((NF, 3))
    s0 = f0 = 0
    for nf, ns in shape:
        if ns == 5:
            count[s0 + 2] = 0
        for s in range(s0, s0 + ns):
            src[s, :count[s]] = rng.choice(NSEG, count[s], replace=False)
        ft[f0:f0 + nf] = (10.0 * np.arange(nf) + 5.0)[rng.permutation(nf)]
        fp[f0:f0 + nf, 0] = 0.0 if one_place else np.arange(nf) + rng.uniform(-0.05, 0.05, nf)
        s0 += ns; f0 += nf
    words = [(nf + 63) // 64 + extra for nf in n_frames]
    return dict(shape=shape, robots=session_frame_robots([NSEG] * R, n_sub, n_frames, words), count=count, src=src, seg=seg, ft=ft, fp=fp,
                fd=rng.normal(0.0, 1.0, (NF, d)), S=S, d=d, words=words)


def per_robot(ctx, P, c):
    """roman_frame_select per robot -> the session's expected outputs by global slot (mask rows in the robots' capacity).  A robot
    without frames selects nothing: its means are the device's 0 / 0, taken from an empty submap of a robot that has frames."""
    rb = c["robots"]
    mask = np.zeros(int(rb["mask_off"][-1] + rb["n_sub"][-1] * rb["mask_words"][-1]), dtype=np.uint64)
    n_sel, span, mean = np.zeros(c["S"], np.int32), np.zeros((c["S"], 2)), np.full((c["S"], c["d"]), np.nan)
    for r in rb:
        s0, ns, f0, nf, mw = int(r["sub0"]), int(r["n_sub"]), int(r["frame0"]), int(r["n_frames"]), int(r["mask_words"])
        if not ns:
            continue
        mean_r = bool(P.want_mean and nf)
        got = ctx.frame_select(frame_select_params(P.thin_dist if P.thin else None, mean_r), c["count"][s0:s0 + ns], c["src"][s0:s0 + ns],
                               c["seg"][int(r["seg0"]):int(r["seg0"]) + NSEG], c["ft"][f0:f0 + nf], c["fp"][f0:f0 + nf], c["fd"][f0:f0 + nf] if mean_r else None)
        rows = mask[int(r["mask_off"]):int(r["mask_off"]) + ns * mw].reshape(ns, mw)
        rows[:, :(nf + 63) // 64] = got.mask
        n_sel[s0:s0 + ns], span[s0:s0 + ns] = got.n_sel, got.span
        if mean_r:
            mean[s0:s0 + ns] = got.mean
            if (got.n_sel == 0).any():
                nothing = got.mean[got.n_sel == 0][0, 0]
    if P.want_mean:
        assert np.isnan(nothing)
        for r in rb[rb["n_frames"] == 0]:
            mean[int(r["sub0"]):int(r["sub0"]) + int(r["n_sub"])] = nothing
    return dict(mask=mask, n_sel=n_sel, span=span, mean=mean)


def lists_of(rb):
    """empty, one slot, every slot, first and last slot of each robot"""
    S = int(rb["sub0"][-1] + rb["n_sub"][-1])
    ends = sorted({int(x) for r in rb if r["n_sub"] for x in (r["sub0"], r["sub0"] + r["n_sub"] - 1)})
    return [[], [S // 2], list(range(S)), ends]


def slot_rows(rb, g):
    """slot g's words in the session's mask"""
    r = rb[(rb["sub0"] <= g) & (g < rb["sub0"] + rb["n_sub"])][0]
    a = int(r["mask_off"]) + (g - int(r["sub0"])) * int(r["mask_words"])
    return slice(a, a + int(r["mask_words"]))


def call(ctx, P, c, lst, buf):
    return ctx.session_frame_select_list(P, c["robots"], c["count"], c["src"], c["seg"], c["ft"], lst, buf["mask"], buf["n_sel"], buf["span"],
                                         frame_pos=c["fp"], frame_desc=c["fd"] if P.want_mean else None, mean=buf["mean"] if P.want_mean else None)


def sentinels(want):
    return {k: np.full(v.shape, SENT[k], dtype=v.dtype) for k, v in want.items()}


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name,thin,one_place", THIN, ids=[t[0] for t in THIN])
@pytest.mark.parametrize("d", [1, 3, 257])
def test_listed_slots_equal_the_per_robot_call_and_unlisted_slots_keep_their_sentinels(ctx, name, thin, one_place, d):
    P = frame_select_params(thin, True)
    selected = dropped = 0
    for k, shape in enumerate(SESSIONS):
        for extra in (0, 2):
            c = session(shape, d, extra, seed=100 * k + d, one_place=one_place)
            want = per_robot(ctx, P, c)
            rb = c["robots"]
            assert np.isnan(want["mean"][want["n_sel"] == 0]).all() and (want["n_sel"][c["count"] == 0] == 0).all()
            selected += int(want["n_sel"].sum()); dropped += int((want["n_sel"] == 1).sum())
            assert not one_place or (want["n_sel"] <= 1).all(), "frames at one position: thinning keeps the first candidate only"
            for lst in lists_of(rb):
                buf = sentinels(want)
                changed = call(ctx, P, c, lst, buf)
                assert changed.shape == (len(lst),) and (changed == 1).all(), (shape, extra, lst, changed)      # (a sentinel count is never the answer)
                for g in range(c["S"]):
                    ref = want if g in lst else sentinels(want)
                    where = "listed" if g in lst else "unlisted"
                    assert same(buf["mask"][slot_rows(rb, g)], ref["mask"][slot_rows(rb, g)]), (shape, extra, lst, g, where, "mask")
                    for key in ("n_sel", "span", "mean"):
                        assert same(buf[key][g], ref[key][g]), (shape, extra, lst, g, where, key)
    assert (dropped >= 1) if one_place else (selected > 50), (selected, dropped)


@pytest.mark.parametrize("want_mean", [True, False], ids=["mean", "no-mean"])
def test_changed_reports_exactly_the_slots_that_differ(ctx, want_mean):
    P = frame_select_params(2.5, want_mean)
    c = session(SESSIONS[1], 3, 2, seed=7)
    want = per_robot(ctx, P, c)
    rb, S = c["robots"], c["S"]
    every = list(range(S))
    # the right answer in place — a NaN mean (an empty submap, a robot without frames) included: nothing changed, nothing is rewritten
    buf = {k: v.copy() for k, v in want.items()}
    assert np.isnan(want["mean"]).any() or not want_mean
    assert not call(ctx, P, c, every, buf).any()
    for k in want:
        assert same(buf[k], want[k]) or (k == "mean" and not want_mean), k
    # one mask bit, one count, one mean column altered, each in a slot of its own
    full = [g for g in every if want["n_sel"][g] > 0]
    a, b, m = full[0], full[1], full[-1]
    buf["mask"][slot_rows(rb, a).start] ^= np.uint64(1)
    buf["n_sel"][b] += 1
    hit = {a, b}
    if want_mean:
        buf["mean"][m, 2] = np.nextafter(buf["mean"][m, 2], np.inf)
        hit.add(m)
    changed = call(ctx, P, c, every, buf)
    assert changed.tolist() == [int(g in hit) for g in every], (changed, hit)
    for k in want:
        assert same(buf[k], want[k]) or (k == "mean" and not want_mean), k
    # a NaN of other bits in the mean row of an empty submap is a change too
    if want_mean:
        e = int(np.nonzero(c["count"] == 0)[0][0])
        buf["mean"][e, 0] = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
        changed = call(ctx, P, c, [e], buf)
        assert changed.tolist() == [1] and same(buf["mean"], want["mean"])


def test_the_device_form_writes_inside_its_slots_only(ctx):
    """Device pointers between guard regions; the list of first and last slots; against the host form."""
    hip = Hip()
    try:
        P = frame_select_params(2.5, True)
        c = session(SESSIONS[0], 257, 2, seed=3)
        want = per_robot(ctx, P, c)
        rb = c["robots"]
        lst = lists_of(rb)[3]
        host = sentinels(want)
        changed_host = call(ctx, P, c, lst, host)
        dev = {k: hip.upload(c[k]) for k in ("count", "src", "seg", "ft", "fp", "fd")}
        out = {k: Guarded(hip, v.size, v.dtype, SENT[k]) for k, v in want.items()}
        ch = Guarded(hip, len(lst), np.int32, -9)
        ctx.session_frame_select_list_dev(P, rb, CAP, dev["count"], dev["src"], dev["seg"], dev["ft"], lst, out["mask"].ptr, out["n_sel"].ptr, out["span"].ptr,
                                          ch.ptr, frame_pos_ptr=dev["fp"], d=c["d"], frame_desc_ptr=dev["fd"], mean_ptr=out["mean"].ptr)
        ctx.sync()
        for k in want:
            assert same(out[k].get(), host[k]), k
        assert np.array_equal(ch.get(), changed_host)
        # L == 0 and R == 0 enqueue nothing
        ctx.session_frame_select_list_dev(P, rb, CAP, dev["count"], dev["src"], dev["seg"], dev["ft"], [], out["mask"].ptr, out["n_sel"].ptr, out["span"].ptr,
                                          ch.ptr, frame_pos_ptr=dev["fp"], d=c["d"], frame_desc_ptr=dev["fd"], mean_ptr=out["mean"].ptr)
        ctx.session_frame_select_list_dev(P, rb[:0], CAP, None, None, None, None, [], None, None, None, None, d=c["d"])
        ctx.sync()
        assert same(out["mask"].get(), host["mask"])
    finally:
        hip.free_all()


def test_error_codes_and_empty_calls_on_a_context(ctx):
    import test_session_grow_frames_abi as abi
    from roman_amd import _abi
    lib = ctx._lib
    abi.check_error_codes(lib, ctx._h)
    for host in (False, True):
        assert abi.Args(lst=()).call(lib, host, ctx._h) == _abi.ROMAN_OK                      # L == 0: nothing is dereferenced
        assert abi.Args(lst=None).call(lib, host, ctx._h) == _abi.ROMAN_OK
        assert abi.Args(lst=(), n_sub=(), n_frames=(), words=()).call(lib, host, ctx._h) == _abi.ROMAN_OK      # R == 0
