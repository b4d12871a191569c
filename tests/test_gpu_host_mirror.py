"""The host-pointer stage calls against their device-pointer forms, byte for byte: submaps_fill, submap_boxes, frame_select,
stacked_sim, grid_gate_sim, grid_gate_aabb and ransac_batch stage the caller's arrays in ONE device block (HostMirror in
roman_hip.hip), call the `_dev` entry and bring the outputs back; the `_dev` form here runs on device arrays this file uploads.

Nothing is compared with a tolerance: both forms launch the same kernels on the same values, so every output is the same bytes.
The shapes are the ones at which the block's layout can go wrong, not the workload's: S = 3 (S0 = 3, S1 = 5) ends every 4-byte
array off an 8-byte boundary in front of an 8-byte one, cap = 9, N = 50 segments, Nf = 70 frames (two mask words, the second
partly used), d = 5, B = 3 RANSAC problems with an odd max_iteration; every optional array is once there and once absent.  The
device outputs start from what the host-pointer form's fresh arrays hold, between guard regions."""
import numpy as np
import pytest

import _frame_desc_oracle as fdo
import _grid_gate_oracle as go
import _ransac_oracle as ro
import _submaps_oracle as so
from _hipmem import Hip
from roman_amd import _abi
from roman_amd.runtime import Context, frame_select_params, grid_gate_params, ransac_record_dtype
from test_gpu_grid_gate import FILL, Guarded

pytestmark = pytest.mark.gpu

S, S0, S1, CAP, N, NF, NF1, D, B = 3, 3, 5, 9, 50, 70, 37, 5, 3
F = 3 + 4 + D
COUNT = np.array([9, 0, 4], dtype=np.int32)                   # a full slot, an empty one, a partly used one
GUARD = {"f": -7.25, "i": -77, "u": 77}


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def dev_out(hip, init):
    """A guarded device array that starts as `init` (a structured array: as its bytes)."""
    init = np.ascontiguousarray(init)
    raw = init.view(np.uint8) if init.dtype.names else init
    g = Guarded(hip, raw.size, raw.dtype, GUARD[raw.dtype.kind])
    if raw.nbytes:
        assert hip.lib.hipMemcpy(g.ptr, raw.ctypes.data, raw.nbytes, 1) == 0
    return g


def same(host, dev, tag):
    for k, h in host.items():
        assert (h is None) == (dev[k] is None), (tag, k)
        if h is not None:
            assert np.asarray(h).tobytes() == np.asarray(dev[k]).tobytes(), f"{tag}: {k} of the host-pointer call differs from the device-pointer call"


def fill_inputs():
    rng = np.random.default_rng(31)
    feats, times, descs = so.random_map(rng, N, F, S)
    src = np.full((S, CAP), -1, dtype=np.int32)
    for s in range(S):
        src[s, :COUNT[s]] = rng.choice(N, COUNT[s], replace=False)
    return feats, times, descs, src, np.arange(N, dtype=np.int64) * 7 + 1000


# ---------------------------------------------------------------------------------------------
# submaps_fill and submap_boxes
# ---------------------------------------------------------------------------------------------
def fill_both(ctx, hip, with_ids, d, want_pool):
    feats, _, descs, src, ids = fill_inputs()
    ids = ids if with_ids else None
    r = ctx.submaps_fill(3, CAP, feats, descs, COUNT, src, seg_ids=ids, desc_dim=d, want_pool=want_pool)
    host = dict(pool=r.pool, ids=r.ids, desc=r.desc)
    rows = S * CAP
    out = dict(pool=dev_out(hip, np.zeros((rows, F))), ids=dev_out(hip, np.full(rows, -1, np.int64)) if with_ids else None,
               desc=dev_out(hip, np.full((S, d), np.nan)) if d else None)
    ctx.submaps_fill_dev(3, CAP, N, F, hip.upload(feats), descs, hip.upload(COUNT), hip.upload(src), out["pool"].ptr,
                         seg_ids_ptr=hip.upload(ids) if with_ids else None, ids_out_ptr=out["ids"].ptr if with_ids else None,
                         desc_dim=d, desc_out_ptr=out["desc"].ptr if d else None)
    ctx.sync()
    dev = {k: (None if v is None else v.get()) for k, v in out.items()}
    if not want_pool:                                         # the device form always writes a pool; the host form then brings none back
        assert r.pool is None
        dev["pool"] = None
    return host, dev


@pytest.mark.parametrize("with_ids,d,want_pool", [(True, D, True), (False, 0, True), (True, 0, False), (False, D, False)])
def test_submaps_fill(ctx, hip, with_ids, d, want_pool):
    host, dev = fill_both(ctx, hip, with_ids, d, want_pool)
    same(host, dev, "submaps_fill")
    if want_pool:
        assert np.any(host["pool"][:CAP] != 0.0) and np.all(host["pool"][CAP:2 * CAP] == 0.0)      # rows were gathered; the empty slot is untouched
    if d:
        assert np.isfinite(host["desc"][0]).all() and np.isnan(host["desc"][1]).all()


def boxes_both(ctx, hip):
    rng = np.random.default_rng(32)
    pool = rng.uniform(-40.0, 40.0, (S * CAP, F))
    T = np.array([go.yaw_pose(rng.uniform(-np.pi, np.pi), rng.uniform(-30, 30, 3)) for _ in range(S)])
    host = dict(box=ctx.submap_boxes(pool, CAP, COUNT, T))
    out = dev_out(hip, np.zeros((S, 6)))
    ctx.submap_boxes_dev(S, F, CAP, hip.upload(pool), hip.upload(COUNT), hip.upload(T), out.ptr)
    ctx.sync()
    return host, dict(box=out.get())


def test_submap_boxes(ctx, hip):
    host, dev = boxes_both(ctx, hip)
    same(host, dev, "submap_boxes")
    assert np.isfinite(host["box"][0]).all() and np.isposinf(host["box"][1, :3]).all()


# ---------------------------------------------------------------------------------------------
# frame_select and stacked_sim
# ---------------------------------------------------------------------------------------------
def select_both(ctx, hip, thin, want_mean):
    rng = np.random.default_rng(33)
    _, _, _, src, _ = fill_inputs()
    ft = 10.0 * np.arange(NF) + 5.0
    first = np.floor(rng.uniform(0.0, 10.0 * NF - 80.0, N)) + 0.25
    seg = np.stack([first, first + np.floor(rng.uniform(10.0, 70.0, N)) + 0.5], axis=1)
    seg[src[0, 0]] = (600.25, 699.5)                                        # submap 0 reaches the last frames: the second mask word
    pos = np.stack([np.arange(NF) + rng.uniform(-0.05, 0.05, NF), rng.uniform(-0.05, 0.05, NF), np.zeros(NF)], axis=1)
    desc = rng.normal(0.0, 1.0, (NF, D))
    P = frame_select_params(2.5 if thin else None, want_mean)
    r = ctx.frame_select(P, COUNT, src, seg, ft, frame_pos=pos if thin else None, frame_desc=desc if want_mean else None)
    host = dict(mask=r.mask, n_sel=r.n_sel, span=r.span, mean=r.mean)
    out = dict(mask=dev_out(hip, np.zeros((S, 2), np.uint64)), n_sel=dev_out(hip, np.zeros(S, np.int32)), span=dev_out(hip, np.zeros((S, 2))),
               mean=dev_out(hip, np.full((S, D), np.nan)) if want_mean else None)
    ctx.frame_select_dev(P, S, CAP, hip.upload(COUNT), hip.upload(src), N, hip.upload(seg), NF, hip.upload(ft), out["mask"].ptr, out["n_sel"].ptr,
                         out["span"].ptr, frame_pos_ptr=hip.upload(pos) if thin else None, d=D if want_mean else 0,
                         frame_desc_ptr=hip.upload(desc) if want_mean else None, mean_ptr=out["mean"].ptr if want_mean else None)
    ctx.sync()
    return host, {k: (None if v is None else v.get()) for k, v in out.items()}


@pytest.mark.parametrize("thin", [False, True])
@pytest.mark.parametrize("want_mean", [False, True])
def test_frame_select(ctx, hip, thin, want_mean):
    host, dev = select_both(ctx, hip, thin, want_mean)
    same(host, dev, "frame_select")
    assert host["n_sel"][0] > 0 and host["n_sel"][1] == 0 and host["mask"][:, 1].any()             # the second mask word is in use


def stacked_both(ctx, hip):
    rng = np.random.default_rng(34)
    desc0, desc1 = rng.normal(0.0, 1.0, (NF, D)), rng.normal(0.0, 1.0, (NF1, D))
    m0 = fdo.pack_mask([np.arange(0, 40), np.array([69]), np.arange(20, 70, 3)], NF)
    m1 = fdo.pack_mask([np.arange(0, 20), np.arange(10, 37), np.array([2]), np.array([], dtype=np.int64), np.arange(0, 37)], NF1)
    host = dict(sim=ctx.stacked_sim(desc0, m0, desc1, m1))
    out = dev_out(hip, np.zeros((S0, S1)))
    ctx.stacked_sim_dev(D, NF, hip.upload(desc0), S0, hip.upload(m0), NF1, hip.upload(desc1), S1, hip.upload(m1), out.ptr)
    ctx.sync()
    return host, dict(sim=out.get())


def test_stacked_sim(ctx, hip):
    host, dev = stacked_both(ctx, hip)
    same(host, dev, "stacked_sim")
    assert np.isneginf(host["sim"][:, 3]).all() and np.isfinite(np.delete(host["sim"], 3, 1)).all()


# ---------------------------------------------------------------------------------------------
# the gates: grid_gate_sim, grid_gate_aabb
# ---------------------------------------------------------------------------------------------
GATE_OUT = dict(dist=(S0, S1), flags=(S0, S1), yaw_deg=(S0, S1), sim=(S0, S1), T_ij=(S0, S1, 4, 4))
COMPACT = dict(pairs=(S0 * S1, 2), T_ref=(S0 * S1, 4, 4), enable=(S0 * S1,))
GATE_DTYPE = dict(flags=np.int32, pairs=np.int32, enable=np.int32, n_todo=np.int32)


def gate_case(form, with_time, with_gt, with_desc=False, with_sim=False):
    """The inputs of one gate call.  form "sim": grid_gate_sim; "aabb": grid_gate_aabb with descriptors, with a given similarity
    or with neither.  -> sides, boxes, the given similarity or None, the gate's parameters, the times or (None, None)."""
    rng = np.random.default_rng(35)
    d = D if with_desc else 0
    a, b = go.random_side(rng, S0, d, with_gt=with_gt), go.random_side(rng, S1, d, with_gt=with_gt)
    boxes = [np.hstack([s["pos"] - rng.uniform(5.0, 25.0, (len(s["pos"]), 3)), s["pos"] + rng.uniform(5.0, 25.0, (len(s["pos"]), 3))]) for s in (a, b)]
    sim_in = rng.uniform(0.2, 0.95, (S0, S1)) if (with_sim or form == "sim") else None
    gate = dict(skip_distance=35.0, desc_dim=d, desc_thresh=0.6 if (d or sim_in is not None) else 0.0, single_robot_lc=with_time, lc_time_thresh=60.0)
    return a, b, boxes, sim_in, gate, [s["time"] if with_time else None for s in (a, b)]


def gate_both(ctx, hip, form, with_time, with_gt, with_desc=False, with_sim=False):
    a, b, boxes, sim_in, gate, tm = gate_case(form, with_time, with_gt, with_desc, with_sim)
    P = grid_gate_params(12.0 if form == "sim" else None, **gate)
    handed = {k: np.full(shape, FILL[k], GATE_DTYPE.get(k, np.float64)) for k, shape in COMPACT.items()}
    if form == "sim":
        r = ctx.grid_gate_sim(P, sim_in, a["pos"], a["T_w"], b["pos"], b["T_w"], time0=tm[0], time1=tm[1], pos_gt0=a["pos_gt"], pos_gt1=b["pos_gt"],
                              **{k: v.copy() for k, v in handed.items()})
    else:
        r = ctx.grid_gate_aabb(P, boxes[0], boxes[1], a["pos"], a["T_w"], b["pos"], b["T_w"], time0=tm[0], time1=tm[1], desc0=a["desc"], desc1=b["desc"],
                               pos_gt0=a["pos_gt"], pos_gt1=b["pos_gt"], sim_in=sim_in, **{k: v.copy() for k, v in handed.items()})
    host = {k: getattr(r, k) for k in list(GATE_OUT) + list(COMPACT)}
    host["n_todo"] = np.array([r.n_todo], np.int32)
    up = lambda x: None if x is None else hip.upload(np.asarray(x, dtype=np.float64))
    out = {k: dev_out(hip, np.zeros(shape, GATE_DTYPE.get(k, np.float64))) for k, shape in GATE_OUT.items()}
    out.update({k: dev_out(hip, v) for k, v in handed.items()})
    out["n_todo"] = dev_out(hip, np.zeros(1, np.int32))
    if form == "sim":
        out["sim"] = dev_out(hip, sim_in)                       # an input of roman_grid_gate_sim_dev: it must come out as it went in
    args = [up(a["pos"]), up(a["T_w"]), up(b["pos"]), up(b["T_w"])] + [out[k].ptr for k in list(GATE_OUT) + list(COMPACT) + ["n_todo"]]
    kw = dict(time0_ptr=up(tm[0]), time1_ptr=up(tm[1]), pos_gt0_ptr=up(a["pos_gt"]), pos_gt1_ptr=up(b["pos_gt"]))
    if form == "sim":
        ctx.grid_gate_sim_dev(P, S0, S1, *args, **kw)
    else:
        ctx.grid_gate_aabb_dev(P, S0, S1, *args, box0_ptr=up(boxes[0]), box1_ptr=up(boxes[1]), sim_in_ptr=up(sim_in) if with_sim else None,
                               desc0_ptr=up(a["desc"]), desc1_ptr=up(b["desc"]), **kw)
    ctx.sync()
    dev = {k: v.get() for k, v in out.items()}
    if form == "aabb" and with_sim:                           # the result's sim is the array handed in; the device's sim output is not written
        assert np.all(dev["sim"] == 0.0) and r.sim.tobytes() == sim_in.tobytes()
        dev["sim"] = sim_in
    return host, dev


def check_gate(host, dev, tag):
    same(host, dev, tag)
    n = int(host["n_todo"][0])
    assert 0 < n < S0 * S1, (tag, n)                          # some pairs are TODO, and some capacity slots stay as handed in
    assert (host["pairs"][n:] == FILL["pairs"]).all() and (host["T_ref"][n:] == FILL["T_ref"]).all() and (host["enable"][n:] == FILL["enable"]).all()


@pytest.mark.parametrize("with_time,with_gt", [(True, True), (False, False)])
def test_grid_gate_sim(ctx, hip, with_time, with_gt):
    check_gate(*gate_both(ctx, hip, "sim", with_time, with_gt), "grid_gate_sim")


AABB = [dict(with_time=True, with_gt=True, with_desc=True), dict(with_time=False, with_gt=False, with_sim=True),
        dict(with_time=True, with_gt=False, with_sim=True), dict(with_time=False, with_gt=True)]


@pytest.mark.parametrize("case", AABB, ids=["desc-time-gt", "sim_in", "sim_in-time", "bare-gt"])
def test_grid_gate_aabb(ctx, hip, case):
    check_gate(*gate_both(ctx, hip, "aabb", **case), "grid_gate_aabb")


# ---------------------------------------------------------------------------------------------
# ransac_batch
# ---------------------------------------------------------------------------------------------
MAX_ITER, KMAX = 201, 7                                       # (an odd number of counts per problem; kmax below the largest inlier count)


def ransac_both(ctx, hip, with_counts):
    # (CPU oracle: 12 inliers, a list cut at kmax; a 3 x 3 problem that stops after 192 of the 201 hypotheses; no inlier at all)
    sets = [ro.planted(n, m, seed, n_in=n_in)[:2] for n, m, seed, n_in in [(12, 12, 100, 12), (3, 3, 100, 3), (4, 7, 101, 3)]]
    pts = np.vstack([x for PQ in sets for x in PQ])
    n1 = np.array([len(p) for p, _ in sets], np.int32); n2 = np.array([len(q) for _, q in sets], np.int32)
    off1 = np.concatenate([[0], np.cumsum(n1 + n2)[:-1]]).astype(np.int64); off2 = off1 + n1
    P = _abi.RomanRansacParams(MAX_ITER, 64, 0.5, 0.5, 0.999, 0)
    r = ctx.ransac_batch(P, pts, off1, n1, off2, n2, kmax=KMAX, counts=True if with_counts else None)
    rec0 = np.zeros(B, dtype=ransac_record_dtype())
    out = dict(assoc=dev_out(hip, np.zeros((B, KMAX, 2), np.int32)), rec=dev_out(hip, rec0),
               counts=dev_out(hip, np.full((B, MAX_ITER), -2, np.int32)) if with_counts else None)
    ctx.ransac_batch_dev(P, hip.upload(pts), off1, n1, off2, n2, KMAX, out["assoc"].ptr, out["rec"].ptr, out["counts"].ptr if with_counts else None)
    ctx.sync()
    rec = out["rec"].get().view(rec0.dtype)
    rows = out["assoc"].get().reshape(B, KMAX, 2)
    host = {f"rec.{f}": r.records[f] for f in rec0.dtype.names}
    dev = {f"rec.{f}": rec[f] for f in rec0.dtype.names}
    for b in range(B):                                        # the result holds a problem's first min(n_assoc, kmax) rows
        host[f"assoc[{b}]"] = r.assoc[b]; dev[f"assoc[{b}]"] = rows[b, :min(int(rec["n_assoc"][b]), KMAX)]
    host["counts"] = r.counts; dev["counts"] = out["counts"].get().reshape(B, MAX_ITER) if with_counts else None
    return host, dev


@pytest.mark.parametrize("with_counts", [True, False])
def test_ransac_batch(ctx, hip, with_counts):
    host, dev = ransac_both(ctx, hip, with_counts)
    same(host, dev, "ransac_batch")
    assert host["rec.n_assoc"].tolist() == [12, 3, 0] and host["rec.n_hyp"].tolist() == [MAX_ITER, 192, MAX_ITER]
    if with_counts:
        assert (host["counts"][1, 192:] == -2).all() and (host["counts"][:, :192] != -2).all()     # entries beyond n_hyp are as handed in


# ---------------------------------------------------------------------------------------------
# one block for every call: grown by the largest, reused by the smallest, reused by the largest
# ---------------------------------------------------------------------------------------------
def test_the_shared_block_grows_and_is_reused(hip):
    """In a fresh context the AABB gate with every optional array (about 6.7 KB of pieces) allocates the block, RANSAC without
    counts (under 1 KB) runs inside it, and the gate again gives the bytes of its first run."""
    ctx = Context(0)
    try:
        first, dev = gate_both(ctx, hip, "aabb", **AABB[0])
        same(first, dev, "first gate")
        same(*ransac_both(ctx, hip, False), "ransac in the gate's block")
        third, _ = gate_both(ctx, hip, "aabb", **AABB[0])
        same(third, first, "the gate after a smaller call")
    finally:
        ctx.close()
