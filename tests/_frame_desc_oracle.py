"""Frame-descriptor submaps restated in NumPy — TEST INFRASTRUCTURE: the expectation for roman_frame_select* and roman_stacked_sim*
(include/roman_hip.h), and the stand-ins the CPU suite runs build_submap_pool(frames=...) / submap_align_pools on.

The arithmetic follows the contract term by term: the thinning distance as sqrt((dx^2 + dy^2) + dz^2), the mean as the selected
rows added one after the other in ascending frame index and divided by their number; only the d-long sums of the cosine are
NumPy's own (their order is free in the contract).

`borderline()` flags an input on which a decision could depend on the last bits of a sum: seeded test inputs carry no flag
(`clean()` raises on one that does: a flagged seed is a test error, never a skip).
"""
import numpy as np

TOL = 1e-9


def pack_mask(sel, Nf):
    """list of index arrays -> (S, ceil(Nf / 64)) uint64, bit f % 64 of word f / 64"""
    W = (Nf + 63) // 64
    m = np.zeros((len(sel), W), dtype=np.uint64)
    for s, idx in enumerate(sel):
        for f in idx:
            m[s, int(f) // 64] |= np.uint64(1) << np.uint64(int(f) % 64)
    return m


def unpack_mask(words):
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    return np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))[0].astype(np.int64)


def _dist(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def frame_select_oracle(count, src, seg_times, frame_times, frame_pos=None, frame_desc=None, thin_dist=None, want_mean=False):
    """-> dict(sel: list of ascending index arrays, mask (S, W) uint64, n_sel (S,) int32, span (S, 2), mean (S, d) or None,
    cand: list of candidate index arrays, steps: list of the thinning distances that were compared)"""
    count = np.asarray(count, np.int32).reshape(-1); S = len(count)
    src = np.asarray(src, np.int32).reshape(S, -1)
    seg_times = np.asarray(seg_times, np.float64).reshape(-1, 2)
    frame_times = np.asarray(frame_times, np.float64).reshape(-1); Nf = len(frame_times)
    sel, cand_all, steps = [], [], []
    span = np.zeros((S, 2))
    for s in range(S):
        rows = src[s, :count[s]]
        lo = seg_times[rows, 0].min() if len(rows) else np.inf                                     # Submap.first_seen [REF roman/map/map.py:125-127]
        hi = seg_times[rows, 1].max() if len(rows) else -np.inf                                    # Submap.last_seen [REF :129-131]
        span[s] = lo, hi
        cand = np.nonzero((frame_times >= lo) & (frame_times <= hi))[0]                            # [REF :218]
        cand_all.append(cand)
        if thin_dist is None:
            sel.append(cand.astype(np.int64))
            continue
        keep, last = [], None
        for f in cand:                                                                             # [REF :236-240]
            if last is not None:
                steps.append(_dist(frame_pos[f], last))
            if last is None or _dist(frame_pos[f], last) >= thin_dist:
                keep.append(f); last = frame_pos[f]
        sel.append(np.array(keep, dtype=np.int64))
    mean = None
    if want_mean:
        frame_desc = np.asarray(frame_desc, np.float64)
        mean = np.full((S, frame_desc.shape[1]), np.nan)
        for s in range(S):
            if len(sel[s]):
                acc = np.zeros(frame_desc.shape[1])
                for f in sel[s]:                                                                   # row after row, as NumPy's mean(axis=0) adds them [REF :219]
                    acc = acc + frame_desc[f]
                mean[s] = acc / len(sel[s])
    return dict(sel=sel, mask=pack_mask(sel, Nf), n_sel=np.array([len(x) for x in sel], dtype=np.int32), span=span, mean=mean,
                cand=cand_all, steps=np.array(steps, dtype=np.float64))


def frame_cosine(desc0, desc1):
    """c(a, b) for every frame pair -> (cosines with the zero guard, norm products)"""
    A, B = np.asarray(desc0, np.float64), np.asarray(desc1, np.float64)
    norm_prod = np.sqrt(np.sum(A * A, axis=1))[:, None] * np.sqrt(np.sum(B * B, axis=1))[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (A @ B.T) / norm_prod
    c[norm_prod <= 1e-9] = 0.0                                                                     # [REF roman/map/map.py:159-161]
    return c, norm_prod


def stacked_sim_oracle(desc0, sel0, desc1, sel1):
    """sim[i][j] = max over a in sel0[i], b in sel1[j] of c(a, b); -inf for an empty side.  sel: index arrays or mask words."""
    c, _ = frame_cosine(desc0, desc1)
    sim = np.full((len(sel0), len(sel1)), -np.inf)
    for i, a in enumerate(sel0):
        for j, b in enumerate(sel1):
            if len(a) and len(b):
                sim[i, j] = c[np.ix_(a, b)].max()
    return sim


def borderline(count, src, seg_times, frame_times, frame_pos=None, thin_dist=None):
    """Flags of the selection (empty list: unambiguous): a candidate test within 1e-9 of a span end, a thinning distance within
    1e-9 of thin_dist."""
    o = frame_select_oracle(count, src, seg_times, frame_times, frame_pos, None, thin_dist)
    flags = []
    t = np.asarray(frame_times, np.float64).reshape(-1)
    for s, (lo, hi) in enumerate(o["span"]):
        for end in (lo, hi):
            if np.isfinite(end) and np.any(np.abs(t - end) <= TOL):
                flags.append(f"submap {s}: a frame time within {TOL} of a span end")
    if thin_dist is not None and len(o["steps"]) and np.any(np.abs(o["steps"] - thin_dist) <= TOL):
        flags.append(f"a thinning distance within {TOL} of thin_dist")
    return flags


def borderline_sim(desc0, sel0, desc1, sel1, desc_thresh=None):
    """Flags of the similarity: a sim within 1e-9 of desc_thresh, a norm product within 1e-12 of 1e-9."""
    flags = []
    _, norm_prod = frame_cosine(desc0, desc1)
    if norm_prod.size and np.any(np.abs(norm_prod - 1e-9) <= 1e-12):
        flags.append("a norm product within 1e-12 of 1e-9")
    if desc_thresh is not None:
        sim = stacked_sim_oracle(desc0, sel0, desc1, sel1)
        if np.any(np.abs(sim[np.isfinite(sim)] - desc_thresh) <= TOL):
            flags.append(f"a sim within {TOL} of desc_thresh")
    return flags


def clean(flags, what):
    if flags:
        raise AssertionError(f"{what}: borderline input, choose another seed: {flags[:3]}")


def frame_descriptors(rng, Nf, d, walk=0.35):
    """Seeded frame descriptors that drift along the trajectory (a random walk on a positive-biased start): frames close in time
    are similar, frames far apart are not — the descriptor gate then has pairs on both sides of its threshold."""
    x = rng.normal(0.0, 1.0, d) + 0.5
    out = np.zeros((Nf, d))
    for f in range(Nf):
        x = x + walk * rng.normal(0.0, 1.0, d)
        out[f] = x
    return out


def golden_cases():
    """tests/golden/frame_desc_golden.npz (the reference's own submaps_from_roman_map and Submap.similarity; generator:
    tests/golden/make_frame_desc_golden.py) -> (shared dict, list of case dicts)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_desc_golden.npz"), allow_pickle=False)
    shared = {k: z[k] for k in ("feats", "times", "ids", "trajectory", "traj_times", "frame_desc", "frame_desc_b")}
    shared["kw"] = eval(str(z["kw"]), {"inf": np.inf})
    cases = []
    for name in [str(n) for n in z["names"]]:
        n = int(z[f"{name}/n_submaps"])
        dist = float(z[f"{name}/frame_descriptor_dist"])
        cases.append(dict(name=name, mode=str(z[f"{name}/mode"]), frame_descriptor_dist=None if np.isnan(dist) else dist,
                          sm_id=z[f"{name}/sm_id"], src=[z[f"{name}/src_{q}"] for q in range(n)], sel=[z[f"{name}/sel_{q}"] for q in range(n)],
                          mean=z[f"{name}/mean"], mean_b=z[f"{name}/mean_b"], sim=z[f"{name}/sim"]))
    return shared, cases


# ---------------------------------------------------------------------------------------------
# stand-ins for runtime.Context on a box without a GPU (in the style of tests/_stub_context.py): the raw addresses the real
# entries take (of torch CPU tensors), the oracle above, the results written through the pointers
# ---------------------------------------------------------------------------------------------
class FrameCallsMixin:
    def frame_select_dev(self, fp, S, cap, count_ptr, src_ptr, N, seg_times_ptr, Nf, frame_times_ptr, mask_ptr, n_sel_ptr, span_ptr,
                         frame_pos_ptr=None, d=0, frame_desc_ptr=None, mean_ptr=None):
        from _stub_context import _view
        assert not fp.reserved[0] and not fp.reserved[1]
        self.frame_selects = getattr(self, "frame_selects", 0) + 1
        W = (Nf + 63) // 64
        o = frame_select_oracle(_view(count_ptr, (S,), np.int32), _view(src_ptr, (S, cap), np.int32), _view(seg_times_ptr, (N, 2), np.float64),
                                _view(frame_times_ptr, (Nf,), np.float64), _view(frame_pos_ptr, (Nf, 3), np.float64) if fp.thin else None,
                                _view(frame_desc_ptr, (Nf, d), np.float64) if fp.want_mean else None, fp.thin_dist if fp.thin else None, bool(fp.want_mean))
        _view(mask_ptr, (S, W), np.uint64)[:] = o["mask"]; _view(n_sel_ptr, (S,), np.int32)[:] = o["n_sel"]
        _view(span_ptr, (S, 2), np.float64)[:] = o["span"]
        if fp.want_mean:
            _view(mean_ptr, (S, d), np.float64)[:] = o["mean"]

    def stacked_sim_dev(self, d, Nf0, desc0_ptr, S0, mask0_ptr, Nf1, desc1_ptr, S1, mask1_ptr, sim_ptr):
        from _stub_context import _view
        self.stacked_sims = getattr(self, "stacked_sims", 0) + 1
        if hasattr(self, "order"):
            self.order.append("stacked_sim")
        m0 = _view(mask0_ptr, (S0, (Nf0 + 63) // 64), np.uint64); m1 = _view(mask1_ptr, (S1, (Nf1 + 63) // 64), np.uint64)
        _view(sim_ptr, (S0, S1), np.float64)[:] = stacked_sim_oracle(_view(desc0_ptr, (Nf0, d), np.float64), [unpack_mask(m) for m in m0],
                                                                    _view(desc1_ptr, (Nf1, d), np.float64), [unpack_mask(m) for m in m1])

    def grid_gate_sim_dev(self, gp, S0, S1, pos0, T_w0, pos1, T_w1, dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, n_todo,
                          time0_ptr=None, time1_ptr=None, pos_gt0_ptr=None, pos_gt1_ptr=None):
        """The gate of tests/_grid_gate_oracle.py without descriptors, its classes re-derived from the similarity handed in."""
        import _grid_gate_oracle as go
        from _stub_context import _view
        assert gp.desc_dim == 0
        self.gates = getattr(self, "gates", 0) + 1
        if hasattr(self, "order"):
            self.order.append("gate")
        side = lambda S, pos, gt, T, tm: dict(pos=_view(pos, (S, 3), np.float64), pos_gt=_view(gt, (S, 3), np.float64) if gt else None,
                                              T_w=_view(T, (S, 4, 4), np.float64), time=_view(tm, (S,), np.float64), desc=None)
        a, b = side(S0, pos0, pos_gt0_ptr, T_w0, time0_ptr), side(S1, pos1, pos_gt1_ptr, T_w1, time1_ptr)
        o = go.grid_gate_oracle(a, b, gp.radius, gp.skip_distance, 0.0, bool(gp.single_robot_lc), gp.lc_time_thresh)
        s = _view(sim, (S0, S1), np.float64)
        before = s.copy()
        nearby, skip = (o["flags"] & go.NEARBY) != 0, (o["flags"] & go.SKIP) != 0
        gated = ~skip & (s < gp.desc_thresh)
        todo = ~skip & ~gated
        ti, tj = np.nonzero(todo)
        en = np.ones(len(ti), np.int32)
        if gp.single_robot_lc:
            en[np.abs(a["time"][ti] - b["time"][tj]) < gp.lc_time_thresh] = 0
        B, n = S0 * S1, len(ti)
        _view(dist, (S0, S1), np.float64)[:] = o["dist"]
        _view(flags, (S0, S1), np.int32)[:] = nearby * go.NEARBY + skip * go.SKIP + gated * go.GATED + todo * go.TODO
        _view(yaw, (S0, S1), np.float64)[:] = o["yaw_deg"]; _view(T_ij, (S0, S1, 4, 4), np.float64)[:] = o["T_ij"]
        _view(pairs, (B, 2), np.int32)[:n] = np.stack([ti, tj], axis=1); _view(T_ref, (B, 4, 4), np.float64)[:n] = o["T_ij"][ti, tj]
        _view(enable, (B,), np.int32)[:n] = en; _view(n_todo, (1,), np.int32)[0] = n
        assert np.array_equal(s, before)
