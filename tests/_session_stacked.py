"""Stacked frame descriptors in the session call — TEST INFRASTRUCTURE shared by the session-stacked tests.

`session_stacked_oracle()` is the expectation for roman_session_stacked_sim*: tests/_frame_desc_oracle.stacked_sim_oracle per block
over the views' frame ranges and mask words, concatenated.  `SessionStackedStubContext` adds roman_session_stacked_sim_dev and the
`sim_in` form of the session gate to the stand-in contexts (through raw addresses of host memory), so that submap_align_session runs
the stacked mode without a GPU — and the per-block calls of submap_align_pools it is compared with run on the same stand-in."""
import numpy as np

import _frame_desc_oracle as fo
import _grid_gate_oracle as go
import _session as ss
from _stub_context import _view


def view_masks(mask_words, mask_off, n, frame_n):
    """The (n, ceil(frame_n / 64)) mask rows of a view out of the session's words."""
    W = (int(frame_n) + 63) // 64
    lo = int(mask_off)
    return np.asarray(mask_words, dtype=np.uint64).reshape(-1)[lo:lo + n * W].reshape(n, W)


def session_stacked_oracle(desc, mask_words, frame_lo, frame_n, mask_off, sub_off, blocks):
    """-> (sim (pair_off[nb],) float64: block b row-major at pair_off[b], the per-block (n0, n1) matrices)."""
    per = []
    for r0, r1, _, _ in np.asarray(blocks).reshape(-1, 4).tolist():
        side = []
        for r in (r0, r1):
            n = int(sub_off[r + 1] - sub_off[r])
            rows = view_masks(mask_words, mask_off[r], n, frame_n[r]) if n else np.zeros((0, 0), np.uint64)
            side.append((np.asarray(desc)[int(frame_lo[r]):int(frame_lo[r]) + int(frame_n[r])], [fo.unpack_mask(m) for m in rows]))
        per.append(fo.stacked_sim_oracle(side[0][0], side[0][1], side[1][0], side[1][1]))
    return (np.concatenate([m.reshape(-1) for m in per]) if per else np.zeros(0)), per


def gate_from_sim(o, sim, sub_off, blocks, desc_thresh, time, lc_time_thresh):
    """The classes and the compact outputs of a session gate re-derived from a given similarity: `o` is tests/_session.
    session_gate_oracle() without descriptors (distance, skip, nearby, transforms)."""
    flags = o["flags"]
    nearby, skip = (flags & go.NEARBY) != 0, (flags & go.SKIP) != 0
    gated = ~skip & (sim < desc_thresh)
    todo = ~skip & ~gated
    pairs, T_ref, enable, todo_off, at = [], [], [], [0], 0
    for r0, r1, lc, _ in np.asarray(blocks).reshape(-1, 4).tolist():
        n0, n1 = int(sub_off[r0 + 1] - sub_off[r0]), int(sub_off[r1 + 1] - sub_off[r1])
        ti, tj = np.nonzero(todo[at:at + n0 * n1].reshape(n0, n1))
        gi, gj = ti + int(sub_off[r0]), tj + int(sub_off[r1])
        pairs.append(np.stack([gi, gj], axis=1)); T_ref.append(o["T_ij"][at:at + n0 * n1][ti * n1 + tj])
        en = np.ones(len(ti), np.int32)
        if lc:
            en[np.abs(time[gi] - time[gj]) < lc_time_thresh] = 0
        enable.append(en); todo_off.append(todo_off[-1] + len(ti)); at += n0 * n1
    cat = lambda xs, tail, dt: np.concatenate(xs).astype(dt) if xs else np.zeros((0,) + tail, dt)
    return dict(flags=(nearby * go.NEARBY + skip * go.SKIP + gated * go.GATED + todo * go.TODO).astype(np.int32), pairs=cat(pairs, (2,), np.int32),
                T_ref=cat(T_ref, (4, 4), np.float64), enable=cat(enable, (), np.int32), todo_off=np.array(todo_off, dtype=np.int32))


class SessionStackedStubContext(fo.FrameCallsMixin, ss.SessionStubContext):
    """SessionStubContext plus stacked_sim_dev / grid_gate_sim_dev (the per-block reference), session_stacked_sim_dev and the
    session gate over a given similarity."""

    def __init__(self, dim=3):
        super().__init__(dim)
        self.session_stacked_sims = 0

    def session_stacked_sim_dev(self, d, Nf, desc_ptr, mask_ptr, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off,
                                frame_lo_ptr, frame_n_ptr, mask_off_ptr, sub_off_ptr, blocks_ptr, pair_off_ptr, sim_ptr):
        self.session_stacked_sims += 1; self.order.append("session_stacked_sim")
        R, nb = len(sub_off) - 1, len(blocks)
        for host, dev_ptr, dt in ((frame_lo, frame_lo_ptr, np.int32), (frame_n, frame_n_ptr, np.int32), (mask_off, mask_off_ptr, np.int64),
                                  (sub_off, sub_off_ptr, np.int32), (blocks, blocks_ptr, np.int32), (pair_off, pair_off_ptr, np.int64)):
            host = np.asarray(host)
            assert host.dtype == dt and np.array_equal(_view(dev_ptr, host.shape, dt), host), "the device copy of a table differs from the host copy"
        assert len(frame_lo) == len(frame_n) == len(mask_off) == R and len(pair_off) == nb + 1
        counts = np.diff(sub_off)
        assert np.array_equal(pair_off, ss.tables(counts.tolist(), [tuple(b[:3]) for b in np.asarray(blocks).tolist()])[2])
        assert (np.asarray(frame_lo) >= 0).all() and (np.asarray(frame_lo, np.int64) + frame_n <= Nf).all() and (np.asarray(mask_off) >= 0).all()
        words = int(max([int(mask_off[r]) + int(counts[r]) * ((int(frame_n[r]) + 63) // 64) for r in range(R)], default=0))
        self.frame_table_rows, self.mask_words = int(Nf), words
        self.view_ranges = [(int(frame_lo[r]), int(frame_n[r]), int(mask_off[r])) for r in range(R)]
        desc = _view(desc_ptr, (Nf, d), np.float64) if Nf else np.zeros((0, d))
        mask = _view(mask_ptr, (words,), np.uint64) if words else np.zeros(0, np.uint64)
        sim, _ = session_stacked_oracle(desc, mask, frame_lo, frame_n, mask_off, sub_off, blocks)
        _view(sim_ptr, (int(pair_off[-1]),), np.float64)[:] = sim

    def session_gate_dev(self, gp, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos, T_w,
                         dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, time_ptr=None, desc_ptr=None, pos_gt_ptr=None, has_gt_ptr=None,
                         sim_in_ptr=None):
        if sim_in_ptr is None:
            return super().session_gate_dev(gp, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos, T_w,
                                            dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, time_ptr, desc_ptr, pos_gt_ptr, has_gt_ptr)
        assert gp.desc_dim == 0, "with a given similarity desc_dim must be 0"
        total = int(pair_off[-1])
        given = _view(sim_in_ptr, (total,), np.float64).copy()
        thresh = gp.desc_thresh
        gp.desc_thresh = 0.0                                 # (the gate without descriptors: everything but the similarity's classes)
        try:
            super().session_gate_dev(gp, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos, T_w,
                                     dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, time_ptr, None, pos_gt_ptr, has_gt_ptr)
        finally:
            gp.desc_thresh = thresh
        self.order[-1] = "session_gate_sim"
        _view(sim, (total,), np.float64)[:] = given          # (sim and sim_in may be one buffer: it leaves as it came)
        S = int(sub_off[-1])
        o = dict(flags=_view(flags, (total,), np.int32).copy(), T_ij=_view(T_ij, (total, 4, 4), np.float64).copy())
        r = gate_from_sim(o, given, sub_off, blocks, thresh, _view(time_ptr, (S,), np.float64) if time_ptr else np.zeros(S), gp.lc_time_thresh)
        n = int(r["todo_off"][-1])
        _view(flags, (total,), np.int32)[:] = r["flags"]
        _view(pairs, (total, 2), np.int32)[:n] = r["pairs"]; _view(T_ref, (total, 4, 4), np.float64)[:n] = r["T_ref"]
        _view(enable, (total,), np.int32)[:n] = r["enable"]; _view(todo_off, (len(blocks) + 1,), np.int32)[:] = r["todo_off"]
        assert np.array_equal(_view(sim_in_ptr, (total,), np.float64), given, equal_nan=True)
