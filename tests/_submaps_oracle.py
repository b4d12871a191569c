"""The contract of roman_submaps*  restated in NumPy — TEST INFRASTRUCTURE (tests/test_submaps_cpu.py,
tests/test_gpu_submaps.py, tools/gpu_submaps.py).

It states the radius mode of the reference's submaps_from_roman_map [REF roman/map/map.py:297-346] over a segment TABLE instead of
segment objects: membership [REF :317-326], the transform into the submap's gravity-aligned frame [REF :328-330], the prune
[REF :332-339] and the mean_semantic descriptor [REF :343-346], with the operation order the C ABI fixes (every product and sum
below is one rounded float64 operation; NumPy's elementwise kernels do not fuse them).

`borderline()` flags an input on which the reference's own arithmetic (BLAS dot products, a matrix product for the transform)
may legitimately decide differently from this restatement: such inputs are kept out of fixtures and generated cases."""
import numpy as np

ST_OK, ST_TRUNCATED = 0, 8
TOL = 1e-9


def _centres(seg_feats, T):
    x, y, z = seg_feats[:, 0], seg_feats[:, 1], seg_feats[:, 2]
    return np.stack([((T[c, 0] * x + T[c, 1] * y) + T[c, 2] * z) + T[c, 3] for c in range(3)], axis=1)


def _tests(seg_feats, seg_times, d, radius):
    """-> (distance to the centre, inside the radius, inside the time window) for every segment of the map"""
    dx, dy, dz = seg_feats[:, 0] - d["pos"][0], seg_feats[:, 1] - d["pos"][1], seg_feats[:, 2] - d["pos"][2]
    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
    near = np.ones(len(seg_feats), bool) if radius is None else dist < radius                      # [REF :323-324]
    in_time = ~((seg_times[:, 0] > d["t_hi"]) | (seg_times[:, 1] < d["t_lo"]))                      # [REF :317-320]
    return dist, near, in_time


def _keys(cen, seg_times, d, prune_by_time):
    if prune_by_time:
        return np.abs((seg_times[:, 0] + seg_times[:, 1]) / 2.0 - d["time"])                       # [REF :334]
    return np.sqrt((cen[:, 0] * cen[:, 0] + cen[:, 1] * cen[:, 1]) + cen[:, 2] * cen[:, 2])        # [REF :336]


def submaps_oracle(seg_feats, seg_times, descs, point_dim=3, max_size=None, cap=None, prune_by_time=False, radius=None,
                   seg_ids=None, desc_dim=0):
    """-> dict(count (S,), src (S, cap) padded with -1, rows: list of (count_s, point_dim + F - 3) arrays, ids: list or None,
    status (S,), desc (S, desc_dim) with NaN rows for empty submaps)."""
    seg_feats = np.asarray(seg_feats, np.float64); seg_times = np.asarray(seg_times, np.float64).reshape(-1, 2)
    N, S = len(seg_feats), len(descs)
    cap = int(max_size if max_size is not None else cap)
    out = dict(count=np.zeros(S, np.int32), src=np.full((S, cap), -1, np.int32), rows=[], ids=None if seg_ids is None else [],
               status=np.zeros(S, np.int32), desc=np.full((S, desc_dim), np.nan))
    for s in range(S):
        d = descs[s]
        _, near, in_time = _tests(seg_feats, seg_times, d, radius)
        members = np.nonzero(near & in_time)[0]                                                    # map order [REF :322-326]
        cen = _centres(seg_feats, np.asarray(d["T_center_odom"], np.float64).reshape(4, 4))
        if max_size is not None:                                                                   # sorted() is stable [REF :338-339]
            key = _keys(cen, seg_times, d, prune_by_time)[members]
            key = np.where(np.isnan(key), np.inf, key)
            members = members[np.argsort(key, kind="stable")]
        elif len(members) > cap:
            out["status"][s] = ST_TRUNCATED
        members = members[:cap]
        n = len(members)
        out["count"][s] = n; out["src"][s, :n] = members
        out["rows"].append(np.hstack([cen[members, :point_dim], seg_feats[members, 3:]]).reshape(n, point_dim + seg_feats.shape[1] - 3))
        if seg_ids is not None:
            out["ids"].append(np.asarray(seg_ids, np.int64)[members])
        if desc_dim and n:
            acc = np.zeros(desc_dim)
            for k in members:                                                                      # rows added in output order [REF :346]
                acc = acc + seg_feats[k, seg_feats.shape[1] - desc_dim:]
            out["desc"][s] = acc / n
    return out


def borderline(seg_feats, seg_times, descs, max_size=None, prune_by_time=False, radius=None, tol=TOL):
    """-> list of human-readable flags (empty: the input is unambiguous): a radius test within `tol` of the radius, a time test
    within `tol` of its bound, or two different-valued keys of one submap within `tol` of each other."""
    seg_feats = np.asarray(seg_feats, np.float64); seg_times = np.asarray(seg_times, np.float64).reshape(-1, 2)
    flags = []
    for s, d in enumerate(descs):
        dist, near, in_time = _tests(seg_feats, seg_times, d, radius)
        if radius is not None and np.any(np.abs(dist - radius) <= tol):
            flags.append(f"submap {s}: a centre within {tol} of the radius")
        for col, bound in ((0, d["t_hi"]), (1, d["t_lo"])):
            if np.isfinite(bound) and np.any(np.abs(seg_times[:, col] - bound) <= tol):
                flags.append(f"submap {s}: a time within {tol} of its bound")
        if max_size is not None:
            members = np.nonzero(near & in_time)[0]
            cen = _centres(seg_feats, np.asarray(d["T_center_odom"], np.float64).reshape(4, 4))
            key = np.sort(_keys(cen, seg_times, d, prune_by_time)[members])
            gap = np.diff(key)
            if np.any((gap > 0) & (gap <= tol)):
                flags.append(f"submap {s}: two different keys within {tol}")
    return flags


def random_map(rng, N, F, S, extent=30.0, t_span=200.0, time_threshold=np.inf, coincide=0):
    """A seeded map table and S centres along a line through it (test generator): centres uniform in a box of +-extent,
    first/last seen around a time that grows with x; every centre a yaw + small tilt pose.  `coincide`: that many segments are
    exact copies (centre and times) of segment 0 — exact key ties."""
    from roman_amd.runtime import submap_desc_dtype
    feats = rng.standard_normal((N, F))
    feats[:, :3] = rng.uniform(-extent, extent, (N, 3)) * np.array([1.0, 1.0, 0.1])
    t0 = (feats[:, 0] + extent) / (2 * extent) * t_span + rng.uniform(-5, 5, N)
    times = np.stack([t0, t0 + rng.uniform(0, 10, N)], axis=1)
    for k in range(1, min(coincide, N - 1) + 1):
        feats[k, :3] = feats[0, :3]; times[k] = times[0]
    descs = np.zeros(S, dtype=submap_desc_dtype())
    xs = np.linspace(-extent * 0.6, extent * 0.6, S) if S > 1 else np.zeros(S)
    for s in range(S):
        yaw = rng.uniform(-np.pi, np.pi)
        T = np.eye(4); c, sn = np.cos(yaw), np.sin(yaw)
        T[:3, :3] = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1.0]])
        T[:3, 3] = [xs[s], rng.uniform(-3, 3), rng.uniform(-0.5, 0.5)]
        descs[s]["pos"] = T[:3, 3]
        descs[s]["T_center_odom"] = np.linalg.inv(T)
        descs[s]["time"] = (xs[s] + extent) / (2 * extent) * t_span
    for s in range(S):
        descs[s]["t_lo"] = descs[s - 1]["time"] - time_threshold if s > 0 else -np.inf
        descs[s]["t_hi"] = descs[s + 1]["time"] + time_threshold if s < S - 1 else np.inf
    return np.ascontiguousarray(feats), np.ascontiguousarray(times), descs


def golden_cases():
    """tests/golden/submaps_golden.npz (the reference's own submaps_from_roman_map over roman_amd.synth.make_map; generator:
    tests/golden/make_submaps_golden.py) -> list of dicts."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "submaps_golden.npz"), allow_pickle=False)
    out = []
    for name in [str(n) for n in z["names"]]:
        kw = eval(str(z[f"{name}/kw"]), {"inf": np.inf})              # repr() of the parameters writes `inf`
        variant = str(z[f"{name}/variant"])
        ids = z[f"{name}/sm_id"]
        out.append(dict(name=name, kw=kw, feats=z["feats"], times=z["times"], ids=z["ids"],
                        trajectory=z[f"trajectory/{variant}"], traj_times=z[f"traj_times/{variant}"], n_centers=int(z[f"{name}/n_centers"]),
                        sm_id=ids, sm_time=z[f"{name}/sm_time"], sm_pose_flu=z[f"{name}/sm_pose_flu"], sm_desc=z[f"{name}/sm_desc"],
                        src=[z[f"{name}/src_{q}"] for q in range(len(ids))], cen=[z[f"{name}/cen_{q}"] for q in range(len(ids))]))
    return out


class OracleSubmapContext:
    """A stand-in for runtime.Context.submaps_dev on a box without a GPU, in the style of tests/_stub_context.py: takes the raw
    addresses the real entry takes (here: of torch CPU tensors), computes with submaps_oracle and writes through the pointers."""
    device = 0

    def __init__(self):
        self.calls, self.syncs = 0, 0

    def sync(self):
        self.syncs += 1

    def submaps_dev(self, P, N, F, feats_ptr, times_ptr, descs, pool_ptr, count_ptr, src_ptr, status_ptr, seg_ids_ptr=None,
                    ids_out_ptr=None, desc_dim=0, desc_out_ptr=None):
        from _stub_context import _view
        self.calls += 1
        S, cap, Fo = len(descs), int(P.cap), int(P.point_dim) + F - 3
        feats = _view(feats_ptr, (N, F), np.float64); times = _view(times_ptr, (N, 2), np.float64)
        ids = _view(seg_ids_ptr, (N,), np.int64) if seg_ids_ptr else None
        o = submaps_oracle(feats, times, descs, point_dim=int(P.point_dim), max_size=int(P.max_size) if P.max_size > 0 else None, cap=cap,
                           prune_by_time=bool(P.prune_by_time), radius=float(P.radius) if P.use_radius else None, seg_ids=ids, desc_dim=desc_dim)
        pool = _view(pool_ptr, (S * cap, Fo), np.float64); count = _view(count_ptr, (S,), np.int32)
        src = _view(src_ptr, (S * cap,), np.int32); status = _view(status_ptr, (S,), np.int32)
        ids_out = _view(ids_out_ptr, (S * cap,), np.int64) if ids_out_ptr else None
        desc = _view(desc_out_ptr, (S, desc_dim), np.float64) if desc_out_ptr else None
        for s in range(S):
            n = int(o["count"][s])
            count[s] = n; status[s] = o["status"][s]
            pool[s * cap:s * cap + n] = o["rows"][s]; src[s * cap:s * cap + n] = o["src"][s, :n]
            if ids_out is not None:
                ids_out[s * cap:s * cap + n] = o["ids"][s]
            if desc is not None and n:
                desc[s] = o["desc"][s]
