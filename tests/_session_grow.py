"""A session whose pools grow — TEST INFRASTRUCTURE shared by tests/test_session_grow_cpu.py and
tests/test_gpu_session_grow.py.

`OracleSessionListContext` is the stand-in whose session_submaps_list_dev is tests/_submaps_oracle.py per LISTED submap, with the
call's pad and `changed` semantics restated: a listed slot is written whole (rows beyond the count cleared to 0.0 / -1 / -1, the
descriptor of an empty one to NaN), an unlisted slot is not touched, and changed[l] compares the slot's bytes before and after.
`GrowingSession` makes R robots' views of one place step by step: every step appends a submap per robot (so the former last
submap's t_hi moves) and table rows, and steps may rewrite a row in place."""
import dataclasses

import numpy as np

import _session as ss
import _session_submaps as sx
import _submaps_oracle as so
from _stub_context import _view

NAN_BITS = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def slot_bytes(cap, g, pool, count, src, status, ids=None, desc=None):
    """Every byte of slot g — count, status, the cap rows of src, ids and pool, the descriptor row — as one bytes object."""
    parts = [count[g:g + 1], status[g:g + 1], src.reshape(-1)[g * cap:(g + 1) * cap], pool[g * cap:(g + 1) * cap]]
    if ids is not None:
        parts.append(ids.reshape(-1)[g * cap:(g + 1) * cap])
    if desc is not None:
        parts.append(desc[g])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


class OracleSessionListContext(sx.OracleSessionSubmapContext):
    """OracleSessionSubmapContext plus session_submaps_list_dev over the raw addresses the real entry takes."""

    def __init__(self):
        super().__init__()
        self.list_calls, self.lists = 0, []

    def session_submaps_list_dev(self, P, F, seg_off, feats_ptr, times_ptr, sub_off, descs, lst, pool_ptr, count_ptr, src_ptr, status_ptr, seg_ids_ptr=None,
                                 ids_out_ptr=None, desc_dim=0, desc_out_ptr=None, changed_ptr=None):
        self.list_calls += 1
        lst = np.asarray(lst, dtype=np.int32).reshape(-1)
        self.lists.append(lst.copy())
        cap, Fo, S, N = int(P.cap), int(P.point_dim) + F - 3, int(sub_off[-1]), int(seg_off[-1])
        assert seg_off.dtype == np.int64 and sub_off.dtype == np.int32 and seg_off[0] == 0 and sub_off[0] == 0 and len(descs) == S
        assert (np.diff(lst) > 0).all() and (len(lst) == 0 or (lst[0] >= 0 and lst[-1] < S)), "the list is not strictly ascending inside the session"
        feats = _view(feats_ptr, (N, F), np.float64); times = _view(times_ptr, (N, 2), np.float64)
        seg_ids = _view(seg_ids_ptr, (N,), np.int64) if seg_ids_ptr else None
        pool = _view(pool_ptr, (S * cap, Fo), np.float64); count = _view(count_ptr, (S,), np.int32)
        src = _view(src_ptr, (S * cap,), np.int32); status = _view(status_ptr, (S,), np.int32)
        ids = _view(ids_out_ptr, (S * cap,), np.int64) if ids_out_ptr else None
        desc = _view(desc_out_ptr, (S, desc_dim), np.float64) if desc_out_ptr else None
        changed = _view(changed_ptr, (len(lst),), np.int32) if changed_ptr and len(lst) else None
        for l, g in enumerate(lst.tolist()):
            r = int(np.searchsorted(sub_off, g, side="right")) - 1
            n0, n1 = int(seg_off[r]), int(seg_off[r + 1])
            o = so.submaps_oracle(feats[n0:n1], times[n0:n1], descs[g:g + 1], point_dim=int(P.point_dim), max_size=int(P.max_size) if P.max_size > 0 else None,
                                  cap=cap, prune_by_time=bool(P.prune_by_time), radius=float(P.radius) if P.use_radius else None,
                                  seg_ids=None if ids is None else seg_ids[n0:n1], desc_dim=desc_dim)
            was = slot_bytes(cap, g, pool, count, src, status, ids, desc)
            n = int(o["count"][0])
            count[g] = n; status[g] = o["status"][0]
            rows = slice(g * cap, g * cap + n); pad = slice(g * cap + n, (g + 1) * cap)
            pool[rows] = o["rows"][0]; pool[pad] = 0.0
            src[rows] = o["src"][0, :n]; src[pad] = -1
            if ids is not None:
                ids[rows] = o["ids"][0]; ids[pad] = -1
            if desc is not None:
                desc[g] = o["desc"][0] if n else NAN_BITS
            if changed is not None:
                changed[l] = int(slot_bytes(cap, g, pool, count, src, status, ids, desc) != was)


D = 16
VIEWS = [dict(keep=1.0, first_pose=0, last_pose=None), dict(keep=0.8, first_pose=3, last_pose=None), dict(keep=0.9, first_pose=0, last_pose=19)]


class GrowingSession:
    """R robots' views of one place (tests/_session.robot_view), cut back to `steps` stages: at stage k robot r holds its first
    S_r - (steps - 1 - k) centres — the poses in front of the next centre —, and its first N_r - 5 * (steps - 1 - k) table rows.
    The arrays are the session's own: edit() rewrites a row for this and every later stage."""

    def __init__(self, reg, R, params, steps=5, n_segments=90, n_poses=24, dt=8.0, seed=31):
        from roman_amd import synth
        from roman_amd.align.submaps import MapTable, submap_centers
        self.reg, self.R, self.params, self.steps = reg, R, params, steps
        base = synth.make_map(n_segments, D, seed=seed, n_poses=n_poses, dt=dt)
        self.full, self.traj, self.starts = [], [], []
        for r in range(R):
            sg, traj, times = ss.robot_view(*base, r, **VIEWS[r])
            sg = sorted(sg, key=lambda x: x.first_seen)                      # (map order is the order of first sight: appended rows are recent ones)
            t = MapTable.from_segments(reg, sg)
            self.full.append(dataclasses.replace(t, feats=t.feats.copy(), times=t.times.copy(), ids=t.ids.copy()))
            self.traj.append((traj, np.asarray(times, dtype=np.float64)))
            self.starts.append(submap_centers(traj, times, params).index)
            assert len(self.starts[r]) >= steps + 1 and len(t) > 5 * steps, "the map is too small for the stages"

    def rows(self, r, k):
        return len(self.full[r]) - 5 * (self.steps - 1 - k)

    def stage(self, k):
        """-> (tables, centers) of stage k: fresh objects over copies of the session's arrays."""
        from roman_amd.align.submaps import submap_centers
        tables, centers = [], []
        for r in range(self.R):
            back, t = self.steps - 1 - k, self.full[r]
            n = self.rows(r, k)
            tables.append(dataclasses.replace(t, feats=t.feats[:n].copy(), times=t.times[:n].copy(), ids=t.ids[:n].copy()))
            traj, times = self.traj[r]
            poses = len(times) if back == 0 else int(self.starts[r][len(self.starts[r]) - back])
            c = submap_centers(traj[:poses], times[:poses], self.params)
            assert len(c) == len(self.starts[r]) - back
            centers.append(c)
        return tables, centers

    def edit(self, r, row, feats=None, times=None):
        if feats is not None:
            self.full[r].feats[row, :3] = feats
        if times is not None:
            self.full[r].times[row] = times


def differing_slots(old, new):
    """Per robot: bool over the submaps of the NEW pools — True for a new submap, and for an old one of which any byte (count, status,
    src, ids, pool rows, descriptor) differs between the two fresh builds `old` and `new`."""
    out = []
    for a, b in zip(old, new):
        cap, k = b.cap, len(a.count)
        flag = np.ones(len(b.count), dtype=bool)
        args = lambda q: (q.pool.cpu().numpy(), q.count, q.src, q.status, q.ids, q.desc)
        flag[:k] = [slot_bytes(cap, g, *args(a)) != slot_bytes(cap, g, *args(b)) for g in range(k)]
        out.append(flag)
    return out
