"""A growing session whose frame tables stay resident — TEST INFRASTRUCTURE shared by
tests/test_session_grow_frames_cpu.py and tests/test_gpu_session_grow_frames.py.

`FrameListMixin` is the stand-in's session_frame_select_list_dev: tests/_frame_desc_oracle.py per LISTED slot over the robot's ranges
of the session's tensors, all mask_words of the row written (zero beyond the frames), changed[l] from the slot's words, count and mean
bits before and after; an unlisted slot is not touched, so whatever it held — the last step's answer, or the fill of a tensor made
anew — is what the pools show.  Every call is recorded.  `FrameSession` makes three robots step by step: robot 0 has frames but
neither rows nor submaps; robot 1's frame table grows 63 -> 64 -> 65 (a second mask word), its frame times in no order, so that an
appended frame falls into old submaps' spans; robot 2's frames are its trajectory poses, appended at the end."""
import dataclasses

import numpy as np

import _frame_desc_oracle as fo
import _session_grow as sg
from _stub_context import _view

FD = 8          # frame descriptor length


class FrameListMixin:
    def session_frame_select_list_dev(self, fp, robots, cap, count_ptr, src_ptr, seg_times_ptr, frame_times_ptr, lst, mask_ptr, n_sel_ptr, span_ptr,
                                      changed_ptr, frame_pos_ptr=None, d=0, frame_desc_ptr=None, mean_ptr=None):
        assert not fp.reserved[0] and not fp.reserved[1] and not robots["reserved"].any()
        lst = np.asarray(lst, dtype=np.int32).reshape(-1)
        self.frame_lists = getattr(self, "frame_lists", []) + [lst.copy()]
        self.frame_robots = robots.copy()
        ends = lambda a, n, per=1: np.concatenate([[0], (robots[a] + robots[n] * per)[:-1]])
        for a, n, per in (("seg0", "n_seg", 1), ("sub0", "n_sub", 1), ("frame0", "n_frames", 1), ("mask_off", "n_sub", robots["mask_words"])):
            assert (robots[a] >= ends(a, n, per)).all(), "robot ranges are not ascending and disjoint"
        assert (robots["mask_words"] >= (robots["n_frames"] + 63) // 64).all()
        S = int(robots["sub0"][-1] + robots["n_sub"][-1]); NF = int(robots["frame0"][-1] + robots["n_frames"][-1])
        N = int(robots["seg0"][-1] + robots["n_seg"][-1]); words = int(robots["mask_off"][-1] + robots["n_sub"][-1] * robots["mask_words"][-1])
        assert (np.diff(lst) > 0).all() and (len(lst) == 0 or (lst[0] >= 0 and lst[-1] < S)), "the list is not strictly ascending inside the session"
        if not len(lst):
            return
        count, src = _view(count_ptr, (S,), np.int32), _view(src_ptr, (S, cap), np.int32)
        seg = _view(seg_times_ptr, (N, 2), np.float64)
        ft = _view(frame_times_ptr, (NF,), np.float64) if NF else np.zeros(0)
        pos = _view(frame_pos_ptr, (NF, 3), np.float64) if NF and fp.thin else None
        desc = _view(frame_desc_ptr, (NF, d), np.float64) if NF and fp.want_mean else None
        mask = _view(mask_ptr, (words,), np.uint64) if words else np.zeros(0, np.uint64)
        n_sel, span = _view(n_sel_ptr, (S,), np.int32), _view(span_ptr, (S, 2), np.float64)
        mean = _view(mean_ptr, (S, d), np.float64) if fp.want_mean else None
        changed = _view(changed_ptr, (len(lst),), np.int32)
        for l, g in enumerate(lst.tolist()):
            r = robots[int(np.nonzero((robots["sub0"] <= g) & (g < robots["sub0"] + robots["n_sub"]))[0][0])]
            s0, f0, nf, mw = int(r["seg0"]), int(r["frame0"]), int(r["n_frames"]), int(r["mask_words"])
            o = fo.frame_select_oracle(count[g:g + 1], src[g:g + 1], seg[s0:s0 + int(r["n_seg"])], ft[f0:f0 + nf], None if pos is None else pos[f0:f0 + nf],
                                       None if desc is None else desc[f0:f0 + nf], fp.thin_dist if fp.thin else None, bool(fp.want_mean))
            row = np.zeros(mw, np.uint64); row[:(nf + 63) // 64] = o["mask"][0]
            at = int(r["mask_off"]) + (g - int(r["sub0"])) * mw
            differs = not np.array_equal(mask[at:at + mw], row) or int(n_sel[g]) != int(o["n_sel"][0])
            mask[at:at + mw] = row; n_sel[g] = o["n_sel"][0]; span[g] = o["span"][0]
            if mean is not None:
                differs = differs or mean[g].tobytes() != o["mean"][0].tobytes()
                mean[g] = o["mean"][0]
            changed[l] = int(differs)


class Ctx(FrameListMixin, fo.FrameCallsMixin, sg.OracleSessionListContext):
    """The growing build's stand-in: the list forms of the submap build and of the frame selection (and the per-robot selection)."""


class OldCtx(fo.FrameCallsMixin, sg.OracleSessionListContext):
    """A context without session_frame_select_list_dev: grow_session_pools reselects per robot."""


def fresh_ctx():
    import _session_submaps as sx
    return type("Fresh", (fo.FrameCallsMixin, sx.OracleSessionSubmapContext), {})()


class FrameSession:
    STEPS = 3

    def __init__(self, reg, params, nf1=(63, 64, 65), fd=FD, seed=5):
        from roman_amd.align.submaps import submap_centers
        self.reg, self.params = reg, params
        self.grow = sg.GrowingSession(reg, 2, params, steps=self.STEPS)
        self.nf1 = nf1
        rng = np.random.default_rng(seed)
        t = self.grow.full[0]
        self.none = dataclasses.replace(t, feats=t.feats[:0].copy(), times=t.times[:0].copy(), ids=t.ids[:0].copy())
        self.no_centers = submap_centers([], [], params)
        self.f0 = self._table(np.arange(5.0), rng, fd)
        # robot 1: frame times over its whole stay, in no order — an appended frame lies inside old submaps' spans
        traj, times = self.grow.traj[0]
        n = max(nf1)
        tt = rng.permutation(np.linspace(times[0] - 20.0, times[-1] + 20.0, n) + 0.123)
        self.f1 = self._table(tt, rng, fd, pos=np.stack([np.interp(tt, times, [np.asarray(T)[k, 3] for T in traj]) for k in range(3)], axis=1))
        # robot 2: its trajectory's poses
        traj, times = self.grow.traj[1]
        self.f2 = self._table(np.asarray(times, dtype=np.float64), rng, fd, pos=np.array([np.asarray(T)[:3, 3] for T in traj]))

    @staticmethod
    def _table(times, rng, fd, pos=None):
        from roman_amd.align.submaps import FrameTable
        n = len(times)
        return FrameTable(np.ascontiguousarray(times, dtype=np.float64), np.ascontiguousarray(rng.normal(0.0, 3.0, (n, 3)) if pos is None else pos, dtype=np.float64),
                          fo.frame_descriptors(rng, n, fd))

    def stage(self, k):
        """-> (tables, centers, frames) of stage k"""
        from roman_amd.align.submaps import FrameTable
        tables, centers = self.grow.stage(k)
        cut = lambda f, n: FrameTable(f.times[:n].copy(), f.pos[:n].copy(), f.desc[:n].copy())
        back = self.STEPS - 1 - k
        starts = self.grow.starts[1]
        n2 = len(self.f2) if back == 0 else int(starts[len(starts) - back])
        return [self.none] + tables, [self.no_centers] + centers, [cut(self.f0, len(self.f0)), cut(self.f1, self.nf1[k]), cut(self.f2, n2)]


def frame_differs(before, want):
    """Per robot: bool over the submaps of `want` — the new ones, and the old ones whose pool bytes, frame mask, frame count or mean
    differ between the two fresh builds."""
    rows = sg.differing_slots([dataclasses.replace(q, desc=None) for q in before], [dataclasses.replace(q, desc=None) for q in want])
    out = []
    for a, b, flag in zip(before, want, rows):
        m, W = len(a.count), b.frame_mask.shape[1]
        old = np.zeros((m, W), np.int64); old[:, :a.frame_mask.shape[1]] = a.frame_mask.cpu().numpy()
        d = (old != b.frame_mask.cpu().numpy()[:m]).any(axis=1) | (a.frame_n != b.frame_n[:m])
        if b.desc is not None:
            d |= (a.desc.view(np.int64) != b.desc[:m].view(np.int64)).any(axis=1)
        out.append(flag | np.concatenate([d, np.ones(len(flag) - m, bool)]))
    return out


def same_frames(got, want):
    """The frame fields of two pools: masks, counts and the frame table's contents."""
    assert np.array_equal(got.frame_n, want.frame_n) and got.frame_n.dtype == want.frame_n.dtype
    assert tuple(got.frame_mask.shape) == tuple(want.frame_mask.shape) and got.frame_mask.dtype == want.frame_mask.dtype
    assert np.array_equal(got.frame_mask.cpu().numpy(), want.frame_mask.cpu().numpy())
    assert tuple(got.frame_desc_dev.shape) == tuple(want.frame_desc_dev.shape) and got.frame_desc_dev.is_contiguous()
    assert got.frame_desc_dev.cpu().numpy().tobytes() == want.frame_desc_dev.cpu().numpy().tobytes()
