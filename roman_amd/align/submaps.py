"""Submaps from a whole map on the device: slice, prune, pack in one call.

The reference's `submap_align()` first turns each robot's map into submaps with `submaps_from_roman_map`
[REF roman/map/map.py:244-357] — for the default radius mode a Python loop over S centres x N segments with a deepcopy per kept
(submap, segment) — and `pack_submaps` then packs every submap's rows again.  Here the map is packed ONCE as a per-segment
table (`MapTable`), the sequential centre scan [REF :300-309] stays on the host (`submap_centers`, S is small), and one device
call (`build_submap_pool` -> roman_submaps_dev) produces the feature pool of all submaps in HBM, in fixed slots of `cap` rows per
submap: exactly what roman_align_batch_dev / roman_align_batch_resident / roman_align_lc_batch_dev consume (`SubmapPool.grid_batch`).
With a `FrameTable` the frame-descriptor modes [REF roman/map/map.py:210-242] run behind it on the same stream (roman_frame_select_dev,
DESIGN.md §4.10): which frames every submap holds, as bit masks that stay on the device, and their mean.
No segment object is copied; `SubmapPool.to_submaps` hands out light views for the host-side callers (`submap_align_grid`, the
writers).

The force_fill_submaps mode [REF :264-295] — overlapping slices of max_size segments of the time-sorted map — is covered too
(DESIGN.md §4.12): its ordering is sequential and small and stays on the host (`fill_centers`), and `build_submap_pool(...,
fill=slices)` gathers the slices with roman_submaps_fill_dev, the gather half of roman_submaps_dev, into the same kind of pool.

torch is used for device memory only; nothing numerical happens here.
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .. import _abi
from ..runtime import frame_select_params, mask_indices, session_frame_robots, submap_desc_dtype
from .batch import AlignmentBatch
from .ransac_reg import RansacReg
from .submap_align import Submap, transform_rm_roll_pitch


@dataclass
class SubmapParams:
    """The fields of [REF roman/map/map.py:165-178] the radius mode reads."""
    max_size: Optional[int] = 40
    radius: Optional[float] = 15.0
    distance: float = 10.0
    time_threshold: float = np.inf
    pruning_method: str = 'time'
    submap_descriptor: Optional[str] = None
    frame_descriptor_dist: Optional[float] = None

    @classmethod
    def from_submap_align_params(cls, p):
        """[REF roman/map/map.py:180-192]"""
        if p.force_fill_submaps:
            raise ValueError("force_fill_submaps slices a time-sorted list on the host; the device call covers the radius mode")
        return cls(max_size=p.submap_max_size, radius=p.submap_radius, distance=p.submap_center_dist,
                   time_threshold=p.submap_center_time, pruning_method=p.submap_pruning_method,
                   submap_descriptor=p.submap_descriptor, frame_descriptor_dist=p.frame_descriptor_dist)


@dataclass
class FillSubmapParams:
    """The fields of [REF roman/map/map.py:165-178] the force_fill_submaps mode reads."""
    max_size: int = 40
    overlap: int = 20
    submap_descriptor: Optional[str] = None
    frame_descriptor_dist: Optional[float] = None

    @classmethod
    def from_submap_align_params(cls, p):
        """[REF roman/map/map.py:180-192]"""
        if not p.force_fill_submaps:
            raise ValueError("force_fill_submaps is not set: SubmapParams.from_submap_align_params serves the radius mode")
        return cls(max_size=p.submap_max_size, overlap=p.submap_overlap, submap_descriptor=p.submap_descriptor,
                   frame_descriptor_dist=p.frame_descriptor_dist)


@dataclass
class SubmapCenters:
    """The S submap centres of one map, in the order the scan found them."""
    index: np.ndarray            # (S,) trajectory index of every centre
    time: np.ndarray             # (S,)
    pose_flu: np.ndarray         # (S, 4, 4) COPIES of the trajectory poses with roll and pitch removed
    T_center_odom: np.ndarray    # (S, 4, 4) inv(pose_gravity_aligned) [REF roman/map/map.py:328]
    t_lo: np.ndarray             # (S,) previous centre's time - time_threshold (-inf for the first) [REF :315-320]
    t_hi: np.ndarray             # (S,) next centre's time + time_threshold (+inf for the last)

    def __len__(self):
        return int(self.index.shape[0])

    def descs(self):
        """-> the roman_submap_desc_t array of the C ABI."""
        d = np.zeros(len(self), dtype=submap_desc_dtype())
        if len(self):
            d["pos"] = self.pose_flu[:, :3, 3]; d["T_center_odom"] = self.T_center_odom
            d["time"] = self.time; d["t_lo"] = self.t_lo; d["t_hi"] = self.t_hi
        return d


def submap_centers(trajectory, times, params) -> SubmapCenters:
    """The sequential centre scan of [REF roman/map/map.py:300-309]: pose i opens a submap when it is the first, lies more than
    `params.distance` from the latest centre, or is more than `params.time_threshold` later.  It fixes S.

    Works on COPIES: the reference stores the trajectory's own pose matrices in its submaps and `pose_gravity_aligned` then
    removes their roll and pitch IN PLACE, so the caller's trajectory comes back changed; here the caller's
    trajectory is NOT flattened — `pose_flu` of the result holds flattened copies (the rotation is all that changes: the
    radius test reads the translation only)."""
    idx = []
    for i, (pose, t) in enumerate(zip(trajectory, times)):
        if i == 0 or np.linalg.norm(np.asarray(pose)[:-1, -1] - np.asarray(trajectory[idx[-1]])[:-1, -1]) > params.distance \
                or (t - times[idx[-1]] > params.time_threshold):
            idx.append(i)
    S = len(idx)
    tm = np.array([times[i] for i in idx], dtype=np.float64)
    flat = np.array([transform_rm_roll_pitch(np.array(trajectory[i], dtype=np.float64)) for i in idx]).reshape(S, 4, 4)
    inv = np.array([np.linalg.inv(T) for T in flat]).reshape(S, 4, 4)
    t_lo = np.concatenate([[-np.inf], tm[:-1] - params.time_threshold])[:S]
    t_hi = np.concatenate([tm[1:] + params.time_threshold, [np.inf]])[-S:] if S else np.zeros(0)
    return SubmapCenters(np.array(idx, dtype=np.int64), tm, flat, inv, t_lo, t_hi)


def fill_centers(table, trajectory, times, fparams):
    """The force_fill_submaps mode of [REF roman/map/map.py:264-295] up to the gather: the segments of `table` in a stable order of
    their reference time (first_seen + last_seen) / 2 (Python's sorted() is stable [REF :267]), cut into slices order[i : i + max_size]
    for i in range(0, N, max_size - overlap) [REF :269-271]; a submap's time is the trajectory time nearest to the mean of its
    slice's reference times [REF :274-278], its pose a flattened COPY of that trajectory pose (as in `submap_centers`: the caller's
    trajectory is not changed).  -> (SubmapCenters, list of (n_s,) int32 index arrays, one per submap, in output order).
    t_lo / t_hi are -inf / +inf: this mode has no time window."""
    max_size, overlap = int(fparams.max_size), int(fparams.overlap)
    step = max_size - overlap
    if step < 1:
        raise ValueError(f"max_size - overlap = {step}: range() needs a step >= 1 [REF roman/map/map.py:269]")
    if max_size < 1:
        raise ValueError("max_size must be >= 1")
    key = (table.times[:, 0] + table.times[:, 1]) / 2.0
    order = np.argsort(key, kind='stable')
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    slices, idx = [], []
    for i in range(0, len(order), step):
        sl = order[i:i + max_size]
        slices.append(sl.astype(np.int32))
        idx.append(int(np.argmin(np.abs(times - np.average(key[sl])))))
    S = len(idx)
    tm = times[idx] if S else np.zeros(0)
    flat = np.array([transform_rm_roll_pitch(np.array(trajectory[i], dtype=np.float64)) for i in idx]).reshape(S, 4, 4)
    inv = np.array([np.linalg.inv(T) for T in flat]).reshape(S, 4, 4)
    return SubmapCenters(np.array(idx, dtype=np.int64), np.array(tm, dtype=np.float64), flat, inv, np.full(S, -np.inf), np.full(S, np.inf)), slices


@dataclass
class MapTable:
    """A whole map as the per-segment table of the C ABI: rows in map order, odom frame."""
    feats: np.ndarray            # (N, 3 + ratio features + descriptor) float64: [x y z | the registration's feature columns behind the point]
    times: np.ndarray            # (N, 2) first_seen, last_seen
    ids: np.ndarray              # (N,) int64
    point_dim: int               # centre components an output row keeps (the registration's dim)
    desc_dim: int                # trailing descriptor columns (0: none)
    invariant: Optional[int] = None   # ROMAN_INV_* of the registration that packed the rows (its column order between point and descriptor);
                                      # None: centres only (a RansacReg) or a table built by other means
    shape_cols: Optional[object] = None    # from_point_clouds only: the segment_clouds.ShapeColumns the device wrote (clouds.minimal_segments reads it)
    shape_status: Optional[np.ndarray] = None   # from_point_clouds only: (N,) int32 ROMAN_SEG_* flags of every segment

    @classmethod
    def from_point_clouds(cls, registration, clouds, center_ref='mean', ctx=None, device=None, volume=None, extent=None):
        """The table of `from_segments(registration, ...)` — same layout, same point_dim, desc_dim and invariant — from the segments'
        POINT CLOUDS (a segment_clouds.SegmentClouds): ONE roman_segment_shapes_dev call writes the centre (center_ref 'mean' or
        'bottom_middle' [REF roman/object/segment.py:266-274]; the reference's SubmapParams holds it and from_submap_align_params never
        sets it, so it is an argument here) and whichever of the ratios, volume and extent the registration's rows hold, at the
        columns `registration.pack` puts them; the descriptor columns, times and ids are the host's.  This replaces the reference's
        per-segment loop of set_center_ref + minimal_data() [REF roman/map/map.py:258-262].  `volume` (N,) / `extent` (N, 3) given:
        they replace the device's columns (the box is UNPINNED against open3d, DESIGN.md §2: a caller with open3d keeps its numbers).
        Refused with ValueError before any context is made: seg_off not ascending from 0 or not ending at P, points not (P, 3)
        float64-convertible, descriptors missing or of another width than the registration reads, volume / extent of the wrong shape."""
        from .segment_clouds import table_from_point_clouds
        return table_from_point_clouds(cls, registration, clouds, center_ref, ctx, device, volume, extent)

    @classmethod
    def from_segments(cls, registration, segments):
        """Packs the map ONCE with `registration.pack` (the row layout of the batch calls), plus times and ids.  The table's point
        is always x y z, whatever the registration's dim.  A RansacReg packs centres only: rows of 3 doubles, desc_dim 0."""
        packed = registration.pack(segments)
        dim = registration.dim
        n = len(segments)
        cen = np.array([np.asarray(s.center, dtype=np.float64).reshape(-1)[:3] for s in segments], dtype=np.float64).reshape(n, 3)
        feats = np.ascontiguousarray(np.hstack([cen, packed[:, dim:]]))
        times = np.array([[s.first_seen, s.last_seen] for s in segments], dtype=np.float64).reshape(n, 2)
        ids = np.array([s.id for s in segments], dtype=np.int64).reshape(n)
        if isinstance(registration, RansacReg):                                  # centres only: rows of 3 doubles, no descriptor
            return cls(feats, times, ids, int(dim), 0)
        P = registration._abi_params()
        d = int(P.cos_feature_dim) if P.invariant != _abi.ROMAN_INV_EUCLIDEAN else 0
        return cls(feats, times, ids, int(dim), d, int(P.invariant))

    def __len__(self):
        return int(self.feats.shape[0])


FRAME_MODES = ('mean_frame_descriptor', 'stacked_frame_descriptors')


@dataclass
class FrameTable:
    """The frames of a whole map, in frame order: what extract_submap_descriptors reads [REF roman/map/map.py:210-214, 228]."""
    times: np.ndarray            # (Nf,) float64
    pos: np.ndarray              # (Nf, 3) float64 trajectory pose[:3, 3]
    desc: np.ndarray             # (Nf, d) float64 frame descriptors

    @classmethod
    def from_map(cls, trajectory, times, descriptors):
        """The ROMANMap fields trajectory, times and descriptors (one each per frame)."""
        t = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
        n = t.shape[0]
        pos = np.ascontiguousarray(np.array([np.asarray(T, dtype=np.float64)[:3, 3] for T in trajectory], dtype=np.float64).reshape(-1, 3))
        if descriptors is None:
            raise ValueError("the map has no frame descriptors")      # [REF roman/map/map.py:212]
        desc = np.ascontiguousarray(np.vstack([np.asarray(x, dtype=np.float64).reshape(1, -1) for x in descriptors])) if n else np.zeros((0, 1))
        if pos.shape[0] != n or desc.shape[0] != n:
            raise ValueError("trajectory, times and descriptors must hold one entry per frame")
        return cls(t, pos, desc)

    def __len__(self):
        return int(self.times.shape[0])


class SegmentView:
    """A segment of the map as a submap holds it: every attribute of the map's segment, the centre in the submap's frame."""
    __slots__ = ("_seg", "centroid")

    def __init__(self, seg, center):
        self._seg = seg
        self.centroid = np.asarray(center, dtype=np.float64).reshape(-1, 1)

    @property
    def center(self):
        return self.centroid

    def __getattr__(self, name):
        if name == "_seg":
            raise AttributeError(name)
        return getattr(self._seg, name)


@dataclass
class SubmapPool:
    """The submaps of one map in HBM: submap s owns rows [s * cap, s * cap + count[s]) of `pool`."""
    pool: object                 # torch tensor (S * cap, F) float64 on the device
    cap: int
    count: np.ndarray            # (S,) int32, host
    src: np.ndarray              # (S, cap) int32 map index of every row (-1 beyond count), host
    ids: np.ndarray              # (S, cap) int64, host
    status: np.ndarray           # (S,) int32 ROMAN_ST_OK / ROMAN_ST_ASSOC_TRUNCATED
    desc: Optional[np.ndarray]   # (S, d) mean_semantic descriptors (NaN rows for empty submaps) or None
    centers: SubmapCenters
    table: MapTable
    desc_dev: Optional[object] = None   # the same descriptors as the call left them on the device: torch tensor (S, d) float64, or None (submap_align_pools reads it)
    descriptor_mode: Optional[str] = None      # the submap_descriptor the pool was built with
    ids_dev: Optional[object] = None           # `ids` as the call left them on the device: torch tensor (S * cap,) int64, one per pool row (submap_align_pools'
                                               # shared-segment removal of self loop closures reads it), or None for a pool built by other means
    # the frame-descriptor modes (build_submap_pool(frames=...)): which of the map's frames every submap holds
    frames: Optional[FrameTable] = None
    frame_mask: Optional[object] = None        # torch tensor (S, ceil(Nf / 64)) int64 on the device: bit f % 64 of word f / 64
    frame_n: Optional[np.ndarray] = None       # (S,) int32 frames selected per submap, host
    frame_desc_dev: Optional[object] = None    # torch tensor (Nf, d) float64 on the device: the frame table's descriptors

    @property
    def nonempty(self):
        """Indices of the submaps that hold a segment (the reference drops the others, [REF roman/map/map.py:341])."""
        return np.nonzero(self.count > 0)[0]

    def offsets(self):
        """(first row, rows) of every non-empty submap."""
        k = self.nonempty
        return k.astype(np.int64) * self.cap, self.count[k].astype(np.int32)

    def grid_batch(self, other, mask=None):
        """The S0 x S1 problems (row-major over the NON-EMPTY submaps of either pool; mask[i, j] False leaves a pair out) over the
        two pools concatenated on the device -> (AlignmentBatch, pool tensor).  The batch carries offsets, counts, pair indices
        and the ids of every pool row; its `feats` is a shape-only placeholder (the rows live on the device), which is what
        pipeline.align_resident(registration, batch, pool) and Context.align_lc_batch_dev(params, pool.data_ptr(), F, batch.off1,
        ...) need.  `other is self` (self loop closures): one pool, no copy."""
        import torch
        same = other is self
        if not same and int(other.pool.shape[1]) != int(self.pool.shape[1]):
            raise ValueError("the two pools have different row widths")
        pool = self.pool if same else torch.cat([self.pool, other.pool], dim=0)
        base1 = 0 if same else int(self.pool.shape[0])
        o0, c0 = self.offsets(); o1, c1 = other.offsets()
        ii, jj = np.meshgrid(np.arange(len(o0)), np.arange(len(o1)), indexing='ij')
        ii, jj = ii.ravel(), jj.ravel()
        if mask is not None:
            keep = np.asarray(mask, dtype=bool).ravel()
            ii, jj = ii[keep], jj[keep]
        ids = self.ids.reshape(-1) if same else np.concatenate([self.ids.reshape(-1), other.ids.reshape(-1)])
        feats = np.broadcast_to(np.float64(0.0), tuple(int(x) for x in pool.shape))
        batch = AlignmentBatch(feats, o0[ii], c0[ii], o1[jj] + base1, c1[jj], pair_index=np.stack([ii, jj], axis=1), ids=ids)
        return batch, pool

    def to_submaps(self, segments) -> List[Submap]:
        """Light `Submap` objects of the non-empty submaps for the host-side callers (the unchanged submap_align_grid, the
        writers): segment views in output order with the transformed centre, plus id (the centre's number, as the reference
        numbers them before it drops the empty ones), time, pose_flu and descriptor.  No segment is copied."""
        cen = self.pool[:, :self.table.point_dim].cpu().numpy()
        out = []
        stacked = self.descriptor_mode == 'stacked_frame_descriptors'
        fmask = self.frame_mask.cpu().numpy().view(np.uint64) if stacked else None
        for s in self.nonempty:
            rows = self.src[s, :self.count[s]]
            c = cen[s * self.cap: s * self.cap + self.count[s]]
            if self.table.point_dim < 3:                                     # the row keeps x y only: z on the host, same operation order
                T = self.centers.T_center_odom[s]; p = self.table.feats[rows, :3]
                z = ((T[2, 0] * p[:, 0] + T[2, 1] * p[:, 1]) + T[2, 2] * p[:, 2]) + T[2, 3]
                c = np.hstack([c, z[:, None]])
            segs = [SegmentView(segments[k], c[r]) for r, k in enumerate(rows)]
            if stacked:                                                      # the (k, d) stack, frames in index order [REF roman/map/map.py:225, 242]
                descriptor = self.frames.desc[mask_indices(fmask[s])].copy()
            else:
                descriptor = None if self.desc is None else self.desc[s].copy()
            out.append(Submap(id=int(s), time=float(self.centers.time[s]), segments=segs, pose_flu=self.centers.pose_flu[s].copy(),
                              descriptor=descriptor))
        return out


def submap_call_params(table: MapTable, params: SubmapParams, cap=None) -> _abi.RomanSubmapParams:
    """SubmapParams -> roman_submap_params_t.  `cap`: rows per slot when max_size is None (default: the whole map)."""
    P = _abi.RomanSubmapParams()
    P.point_dim = table.point_dim
    P.max_size = int(params.max_size) if params.max_size is not None else 0
    if params.max_size is not None and int(params.max_size) < 1:
        raise ValueError("max_size must be None or >= 1")
    P.cap = P.max_size if P.max_size > 0 else int(cap if cap is not None else max(len(table), 1))
    P.prune_by_time = int(params.pruning_method == 'time')                   # [REF roman/map/map.py:333-336]: anything else prunes by distance
    P.use_radius = int(params.radius is not None)
    P.radius = float(params.radius) if params.radius is not None else 0.0
    return P


def _descriptor_width(table, params, frames):
    """What params.submap_descriptor asks of a pool over `table` -> (d: columns of the per-submap descriptor the build writes, 0: none;
    framed: a frame-descriptor mode; mean_frames: its mean).  The refusals of build_submap_pool for the descriptor."""
    d = 0
    if params.submap_descriptor == 'mean_semantic':
        if table.desc_dim <= 0:
            raise ValueError("submap_descriptor 'mean_semantic' needs a registration with semantic descriptors")
        d = table.desc_dim
    elif params.submap_descriptor in FRAME_MODES:
        if frames is None:
            raise ValueError(f"submap_descriptor {params.submap_descriptor!r} needs the map's frames: pass frames=FrameTable.from_map(trajectory, times, descriptors)")
    elif params.submap_descriptor is not None:
        raise ValueError(f"unknown submap_descriptor {params.submap_descriptor!r}")
    framed = params.submap_descriptor in FRAME_MODES
    mean_frames = params.submap_descriptor == 'mean_frame_descriptor'
    if mean_frames:
        d = int(frames.desc.shape[1])
    return d, framed, mean_frames


def build_submap_pool(registration, table: MapTable, centers: SubmapCenters, params, ctx=None, device=None, cap=None,
                      frames: Optional[FrameTable] = None, fill=None) -> SubmapPool:
    """The submaps of `table` around `centers` as a device-resident feature pool: ONE roman_submaps_dev call (membership, prune,
    order, transform, gather, mean_semantic descriptors), then one synchronisation that brings count, src, ids, status and the
    descriptors to the host.  The table is uploaded here (once per call); the pool never leaves the device.

    `frames` (a FrameTable) serves submap_descriptor 'mean_frame_descriptor' / 'stacked_frame_descriptors' with
    params.frame_descriptor_dist [REF roman/map/map.py:210-242]: the frame table goes up once, roman_frame_select_dev runs behind
    roman_submaps_dev on the same stream, and the pool keeps frame_mask, frame_n and frame_desc_dev (the mean mode fills desc /
    desc_dev as mean_semantic does).  A non-empty submap that selects no frame is a ValueError: the reference fails on it.

    `fill` (the slices of `fill_centers`, with its centres as `centers` and a FillSubmapParams as `params`): the force_fill_submaps
    mode [REF roman/map/map.py:264-295].  count and src come from the slices and go up; roman_submaps_fill_dev — the gather half
    of roman_submaps_dev, no membership test, no sort — writes the pool, the ids and the mean_semantic descriptors.  The result
    is an ordinary SubmapPool: the frame modes, to_submaps, grid_batch and submap_align_pools read it as any other."""
    import torch
    ctx = ctx or registration._context()
    dev = torch.device(device if device is not None else f"cuda:{getattr(ctx, 'device', 0)}")
    on_host = dev.type == "cpu"                                              # CPU tensors + a stand-in context (tests)
    if fill is not None:
        if len(fill) != len(centers):
            raise ValueError("fill must hold one slice per centre")
        P = _abi.RomanSubmapParams()
        P.point_dim, P.max_size, P.cap = table.point_dim, int(params.max_size), int(params.max_size)
        if P.cap < 1 or any(len(sl) > P.cap for sl in fill):
            raise ValueError("a slice is longer than max_size")
        if any(len(sl) and (int(np.min(sl)) < 0 or int(np.max(sl)) >= len(table)) for sl in fill):
            raise ValueError("a slice holds an index outside the map")
    else:
        P = submap_call_params(table, params, cap)
    S, N, F = len(centers), len(table), int(table.feats.shape[1])
    d, framed, mean_frames = _descriptor_width(table, params, frames)
    Fo, rows = P.point_dim + F - 3, S * P.cap
    feats = torch.from_numpy(table.feats).to(dev); times = torch.from_numpy(table.times).to(dev); ids = torch.from_numpy(table.ids).to(dev)
    pool = torch.zeros((rows, Fo), dtype=torch.float64, device=dev)
    count = torch.zeros(max(S, 1), dtype=torch.int32, device=dev); status = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
    if fill is None:
        src = torch.full((max(rows, 1),), -1, dtype=torch.int32, device=dev)
    else:                                                                    # the lists are the input here: count and src go up
        src_h = np.full((max(S, 1), P.cap), -1, dtype=np.int32); count_h = np.zeros(max(S, 1), dtype=np.int32)
        for s_, sl in enumerate(fill):
            src_h[s_, :len(sl)] = sl; count_h[s_] = len(sl)
        src = torch.from_numpy(src_h.reshape(-1)).to(dev); count = torch.from_numpy(count_h).to(dev)
    ids_out = torch.full((max(rows, 1),), -1, dtype=torch.int64, device=dev)
    desc = torch.full((max(S, 1), max(d, 1)), float("nan"), dtype=torch.float64, device=dev)
    if framed:
        Nf, W = len(frames), (len(frames) + 63) // 64
        thin = params.frame_descriptor_dist if params.submap_descriptor == 'stacked_frame_descriptors' else None      # [REF roman/map/map.py:216-226]
        f_times = torch.from_numpy(frames.times).to(dev); f_pos = torch.from_numpy(frames.pos).to(dev); f_desc = torch.from_numpy(frames.desc).to(dev)
        f_mask = torch.zeros((max(S, 1), max(W, 1)), dtype=torch.int64, device=dev)
        f_n = torch.zeros(max(S, 1), dtype=torch.int32, device=dev); f_span = torch.zeros((max(S, 1), 2), dtype=torch.float64, device=dev)
    if not on_host:
        torch.cuda.current_stream(dev).synchronize()                         # inputs and cleared outputs are in place before the library's stream touches them
    if fill is not None:
        ctx.submaps_fill_dev(P.point_dim, P.cap, N, F, feats.data_ptr(), centers.descs(), count.data_ptr(), src.data_ptr(), pool.data_ptr(),
                             seg_ids_ptr=ids.data_ptr(), ids_out_ptr=ids_out.data_ptr(), desc_dim=0 if framed else d,
                             desc_out_ptr=desc.data_ptr() if d and not framed else None)
    else:
        ctx.submaps_dev(P, N, F, feats.data_ptr(), times.data_ptr(), centers.descs(), pool.data_ptr(), count.data_ptr(), src.data_ptr(),
                        status.data_ptr(), seg_ids_ptr=ids.data_ptr(), ids_out_ptr=ids_out.data_ptr(), desc_dim=0 if framed else d,
                        desc_out_ptr=desc.data_ptr() if d and not framed else None)
    if framed and S:                                                         # behind it on the same stream: reads the count and src it wrote
        ctx.frame_select_dev(frame_select_params(thin, mean_frames), S, P.cap, count.data_ptr(), src.data_ptr(), N, times.data_ptr(), Nf,
                             f_times.data_ptr(), f_mask.data_ptr(), f_n.data_ptr(), f_span.data_ptr(), frame_pos_ptr=f_pos.data_ptr(),
                             d=int(frames.desc.shape[1]), frame_desc_ptr=f_desc.data_ptr(), mean_ptr=desc.data_ptr() if mean_frames else None)
    ctx.sync()
    count_h = count.cpu().numpy()[:S].copy()
    extra = {}
    if framed:
        n_h = f_n.cpu().numpy()[:S].copy()
        bad = np.nonzero((count_h > 0) & (n_h == 0))[0]
        if len(bad):
            raise ValueError(f"submap {int(bad[0])} holds {int(count_h[bad[0]])} segments but no frame of the map lies in its time span: "
                             "the reference cannot build its frame descriptor")
        extra = dict(frames=frames, frame_mask=f_mask[:S, :W], frame_n=n_h, frame_desc_dev=f_desc)
    return SubmapPool(pool, int(P.cap), count_h, src.cpu().numpy()[:rows].reshape(S, P.cap).copy(),
                      ids_out.cpu().numpy()[:rows].reshape(S, P.cap).copy(), status.cpu().numpy()[:S].copy(),
                      desc.cpu().numpy()[:S, :d].copy() if d else None, centers, table, desc_dev=desc[:S, :d] if d else None,
                      descriptor_mode=params.submap_descriptor, ids_dev=ids_out[:rows], **extra)


def _session_refusals(tables, centers, params, cap, frames, fill):
    """What build_session_pools refuses before anything makes a HIP context (its docstring) -> (tables, centers, frames as lists, the
    session's roman_submap_params_t or None for R == 0, (d, framed, mean_frames) of _descriptor_width)."""
    tables, centers = list(tables), list(centers)
    R = len(tables)
    if fill is not None or isinstance(params, FillSubmapParams) or getattr(params, "force_fill_submaps", False):
        raise ValueError("the session call covers the radius mode: the force_fill_submaps mode orders its slices on the host, use "
                         "build_submap_pool(fill=...) per robot")
    if len(centers) != R:
        raise ValueError("centers must hold one SubmapCenters per table")
    frames = [None] * R if frames is None else list(frames)
    if len(frames) != R:
        raise ValueError("frames must hold one FrameTable per table")
    layout = lambda t: (int(t.feats.shape[1]), int(t.point_dim), int(t.desc_dim), t.invariant)
    if any(layout(t) != layout(tables[0]) for t in tables):
        raise ValueError("the tables differ in row width, point_dim, desc_dim or invariant: one session call packs rows of one layout")
    widths = [_descriptor_width(t, params, f) for t, f in zip(tables, frames)]       # (build_submap_pool's refusals, per robot)
    if len({w for w in widths}) > 1:
        raise ValueError("the robots' frame descriptors differ in length")
    if cap is None and params.max_size is None:
        cap = max([len(t) for t in tables] + [1])
    calls = [submap_call_params(t, params, cap) for t in tables]
    if R == 0:
        return tables, centers, frames, None, (0, False, False)
    return tables, centers, frames, calls[0], widths[0]


def _session_pool_views(tables, centers, frames, params, P, sub_off, d, framed, pool, ids_out, desc, count_h, status_h, src_h, ids_h, desc_h, ft):
    """The R SubmapPools over the session's tensors: pool r's `pool`, `ids_dev` and `desc_dev` are row-slice views, its host fields
    copies of its slices of the arrays read back (ft: per robot the frame-select tensors of the frame-descriptor modes)."""
    out = []
    for r in range(len(tables)):
        lo, hi = int(sub_off[r]), int(sub_off[r + 1])
        extra = {}
        if framed:
            n_h = (ft[r]["n_h"] if "n_h" in ft[r] else ft[r]["n"].cpu().numpy())[:hi - lo].copy()
            bad = np.nonzero((count_h[lo:hi] > 0) & (n_h == 0))[0]
            if len(bad):
                raise ValueError(f"submap {int(bad[0])} holds {int(count_h[lo + bad[0]])} segments but no frame of the map lies in its time span: "
                                 "the reference cannot build its frame descriptor")
            extra = dict(frames=frames[r], frame_mask=ft[r]["mask"][:hi - lo, :ft[r]["W"]], frame_n=n_h, frame_desc_dev=ft[r]["desc"])
        out.append(SubmapPool(pool[lo * P.cap:hi * P.cap], int(P.cap), count_h[lo:hi].copy(), src_h[lo:hi].copy(), ids_h[lo:hi].copy(),
                              status_h[lo:hi].copy(), desc_h[lo:hi].copy() if d else None, centers[r], tables[r],
                              desc_dev=desc[lo:hi, :d] if d else None, descriptor_mode=params.submap_descriptor,
                              ids_dev=ids_out[lo * P.cap:hi * P.cap], **extra))
    return out


def _frame_tensors(torch, dev, frames, centers):
    """Per robot the frame table on the device and cleared frame-select outputs (the frame-descriptor modes of the session builds)."""
    ft = []
    for r, fr in enumerate(frames):
        S_r, W = len(centers[r]), (len(fr) + 63) // 64
        ft.append(dict(W=W, times=torch.from_numpy(fr.times).to(dev), pos=torch.from_numpy(fr.pos).to(dev), desc=torch.from_numpy(fr.desc).to(dev),
                       mask=torch.zeros((max(S_r, 1), max(W, 1)), dtype=torch.int64, device=dev),
                       n=torch.zeros(max(S_r, 1), dtype=torch.int32, device=dev), span=torch.zeros((max(S_r, 1), 2), dtype=torch.float64, device=dev)))
    return ft


def _frame_select_robots(ctx, params, P, tables, frames, seg_off, sub_off, mean_frames, count, src, times, desc, ft):
    """roman_frame_select_dev per robot behind a session build, on the same stream: each reads its robot's count and src."""
    thin = params.frame_descriptor_dist if params.submap_descriptor == 'stacked_frame_descriptors' else None      # [REF roman/map/map.py:216-226]
    for r in range(len(tables)):
        lo, hi, f = int(sub_off[r]), int(sub_off[r + 1]), ft[r]
        if hi > lo:
            ctx.frame_select_dev(frame_select_params(thin, mean_frames), hi - lo, P.cap, count[lo:].data_ptr(), src[lo * P.cap:].data_ptr(), len(tables[r]),
                                 times[int(seg_off[r]):].data_ptr(), len(frames[r]), f["times"].data_ptr(), f["mask"].data_ptr(), f["n"].data_ptr(),
                                 f["span"].data_ptr(), frame_pos_ptr=f["pos"].data_ptr(), d=int(frames[r].desc.shape[1]), frame_desc_ptr=f["desc"].data_ptr(),
                                 mean_ptr=desc[lo:].data_ptr() if mean_frames else None)


def build_session_pools(registration, tables, centers, params, ctx=None, device=None, cap=None, frames=None, fill=None) -> List[SubmapPool]:
    """The submap pools of ALL R robots of a session (one MapTable and one SubmapCenters each) from ONE roman_session_submaps_dev
    call: the R tables go up once, concatenated in robot order; one launch sequence writes every robot's submaps
    into ONE pool tensor — and one ids, count, src, status and descriptor tensor —; one synchronisation brings the small arrays
    back.  Pool r is an ordinary SubmapPool whose `pool`, `ids_dev` and `desc_dev` are row-slice VIEWS of the session's tensors,
    bit for bit what build_submap_pool(registration, tables[r], centers[r], params, cap=<the session's cap>) gives: grid_batch,
    to_submaps and submap_align_pools read it unchanged, and submap_align_session over the list runs on the one allocation
    without concatenating anything.

    One `cap` serves the session: params.max_size, or `cap`, or the largest map's rows.  `frames`: one FrameTable per robot for the
    frame-descriptor modes — roman_frame_select_dev per robot behind the session call, on the same stream, as in build_submap_pool.

    Refused (ValueError, before anything makes a HIP context): `fill=` or params of the force_fill_submaps mode — that mode slices
    on the host, build_submap_pool(fill=...) per robot serves it —, tables of different row width, point_dim, desc_dim or
    invariant, a `centers` or `frames` list whose length is not R, and whatever build_submap_pool refuses per robot."""
    import torch
    tables, centers, frames, P, (d, framed, mean_frames) = _session_refusals(tables, centers, params, cap, frames, fill)
    R = len(tables)
    if R == 0:
        return []
    ctx = ctx or registration._context()
    dev = torch.device(device if device is not None else f"cuda:{getattr(ctx, 'device', 0)}")
    on_host = dev.type == "cpu"                                              # CPU tensors + a stand-in context (tests)
    F = int(tables[0].feats.shape[1])
    seg_off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum([len(c) for c in centers])]).astype(np.int32)
    S, Fo = int(sub_off[-1]), P.point_dim + F - 3
    rows = S * P.cap
    # the concatenated table is made ON the device — one tensor, every robot's rows copied straight into their range: joining the
    # tables on the host first would copy the whole session (hundreds of MB) once more through host memory
    feats = torch.empty((int(seg_off[-1]), F), dtype=torch.float64, device=dev)
    for r, t in enumerate(tables):
        feats[int(seg_off[r]):int(seg_off[r + 1])].copy_(torch.from_numpy(np.ascontiguousarray(t.feats, dtype=np.float64)))
    times = torch.from_numpy(np.ascontiguousarray(np.concatenate([t.times.reshape(-1, 2) for t in tables], axis=0), dtype=np.float64)).to(dev)
    ids = torch.from_numpy(np.ascontiguousarray(np.concatenate([t.ids.reshape(-1) for t in tables]), dtype=np.int64)).to(dev)
    descs = np.concatenate([c.descs() for c in centers])
    pool = torch.zeros((rows, Fo), dtype=torch.float64, device=dev)
    count = torch.zeros(max(S, 1), dtype=torch.int32, device=dev); status = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
    src = torch.full((max(rows, 1),), -1, dtype=torch.int32, device=dev)
    ids_out = torch.full((max(rows, 1),), -1, dtype=torch.int64, device=dev)
    desc = torch.full((max(S, 1), max(d, 1)), float("nan"), dtype=torch.float64, device=dev)
    ft = _frame_tensors(torch, dev, frames, centers) if framed else []
    if not on_host:
        torch.cuda.current_stream(dev).synchronize()                         # inputs and cleared outputs are in place before the library's stream touches them
    ctx.session_submaps_dev(P, F, seg_off, feats.data_ptr(), times.data_ptr(), sub_off, descs, pool.data_ptr(), count.data_ptr(), src.data_ptr(),
                            status.data_ptr(), seg_ids_ptr=ids.data_ptr(), ids_out_ptr=ids_out.data_ptr() if len(ids) else None,     # (no segment at all: no id to write)
                            desc_dim=0 if framed else d, desc_out_ptr=desc.data_ptr() if d and not framed else None)
    if framed:                                                               # behind it on the same stream: each reads its robot's count and src
        _frame_select_robots(ctx, params, P, tables, frames, seg_off, sub_off, mean_frames, count, src, times, desc, ft)
    ctx.sync()
    count_h, status_h = count.cpu().numpy()[:S].copy(), status.cpu().numpy()[:S].copy()
    src_h, ids_h = src.cpu().numpy()[:rows].reshape(S, P.cap), ids_out.cpu().numpy()[:rows].reshape(S, P.cap)
    desc_h = desc.cpu().numpy()[:S, :d] if d else None
    return _session_pool_views(tables, centers, frames, params, P, sub_off, d, framed, pool, ids_out, desc, count_h, status_h, src_h, ids_h, desc_h, ft)


# ---------------------------------------------------------------------------------------------
# a session that GROWS: the tables and the pools stay in HBM, a step builds the new and the changed submaps only
# ---------------------------------------------------------------------------------------------
GROWTH = 1.5                     # capacity of the session's tensors over the need, when they have to be made anew

# the session's tensors: name -> (rows per unit: 1, or 'cap' for the slot tensors; unit: 'seg' table rows or 'sub' submaps; the value a fresh one holds)
_SESSION_TENSORS = dict(feats=(1, 'seg', 0.0), times=(1, 'seg', 0.0), ids=(1, 'seg', 0),
                        pool=('cap', 'sub', 0.0), src=('cap', 'sub', -1), ids_out=('cap', 'sub', -1), count=(1, 'sub', 0), status=(1, 'sub', 0),
                        desc=(1, 'sub', float("nan")))
# ... and of the frame-descriptor modes over a context that selects by list: unit 'frm' frames.  The mask words are
# held apart (`_moved_mask`): a robot's range there is its submaps times its own word capacity
_SESSION_FRAME_TENSORS = dict(f_times=(1, 'frm', 0.0), f_pos=(1, 'frm', 0.0), f_desc=(1, 'frm', 0.0), f_n=(1, 'sub', 0), f_span=(1, 'sub', 0.0))


class SessionPoolsState:
    """What grow_session_pools keeps between two steps of one session: the device tensors of the tables (feats, times, ids) and of
    the outputs (pool, src, ids_out, count, status, desc) — each with room beyond the need, every robot's range next to the one in
    front of it —, per robot the rows and submaps it held and its centre records as bytes, and `src` / `count` on the host.  In the
    frame-descriptor modes over a context with session_frame_select_list_dev also the session's frame tensors —
    f_times, f_pos, f_desc by frame, f_n and f_span by submap, f_mask in rows of a per-robot word capacity —, per robot its frames
    and that capacity, and `span` on the host."""

    def __init__(self):
        self.key = None              # robots, cap, row layout, submap_descriptor: a state serves ONE session
        self.t = {}                  # name -> torch tensor (see _SESSION_TENSORS)
        self.n_rows = None           # per robot: rows of its table
        self.n_sub = None            # per robot: its submaps
        self.descs = None            # per robot: uint8 (S_r, sizeof(roman_submap_desc_t)) as the last call staged them
        self.count_h = None          # (S,) int32 and (S, cap) int32 over the whole session, as read back last
        self.src_h = None
        self.frame = None            # the frame-descriptor modes, per robot: dict(mask, n, mean) device tensors of the last call
        self.n_frames = None         # §4.23, per robot: frames of its table, and the words a mask row of it has room for
        self.mask_words = None
        self.span_h = None           # (S, 2) float64 over the whole session, as read back last
        self.frames_uploaded = 0     # frames the last call uploaded, and slots it listed for the frame selection (of `total`)
        self.frames_listed = 0
        self.listed = 0              # submaps the last call rebuilt, of `total`
        self.total = 0
        self.unfinished = False      # a call moved the session's tensors and raised before it recorded the new layout: the state serves no further call
        self.seconds = {}            # the last call's wall time by part: 'upload' (host rules, moves and table rows), 'device' (the call to its
                                     # synchronisation), 'readback'


def _moved(torch, t, old_off, old_len, new_off, total, per, fill):
    """Tensor `t` with robot r's range of old_len[r] units (of `per` rows each) moved from unit old_off[r] to new_off[r] >= old_off[r]:
    in place from the last robot backwards while `total` units fit, else into a tensor GROWTH times the need (filled with `fill`)."""
    if total * per > int(t.shape[0]):
        new = torch.full((max(int(total * per * GROWTH), 1),) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
        for o, n, k in zip(old_off, new_off, old_len):
            if k:
                new[n * per:(n + k) * per].copy_(t[o * per:(o + k) * per])
        return new
    for o, n, k in reversed(list(zip(old_off, new_off, old_len))):
        if k and n != o:
            t[n * per:(n + k) * per] = t[o * per:(o + k) * per].clone()          # (the ranges may overlap)
    return t


def _grow_frames(torch, dev, state, frames, frames_changed, first, listed, n_rows, n_sub, old_sub, n_frames, sub_off, old_sub_off):
    """The frame half of a growing step before its device call: the frame list — every rule is a necessary
    condition for a slot's selection to change —, the session's frame tensors moved and grown, the appended frames uploaded
    -> (per robot the views _session_pool_views reads, the list, the robots' records, the cleared `changed` of the list, the mask
    word capacities, the frames uploaded).  The caller records n_frames, mask_words, frames_uploaded and span_h in the state with
    the rest of the new layout, when the call has ended."""
    R, t = len(frames), state.t
    d = int(frames[0].desc.shape[1])
    if any(int(f.desc.shape[1]) != d for f in frames):
        raise ValueError("the robots' frame descriptors differ in length")
    fresh = state.n_frames is None                                           # no frame tensor yet (a first call, or the steps so far ran without the entry)
    old_nf, old_mw = ([0] * R, [0] * R) if fresh else (state.n_frames, state.mask_words)
    whole = [fresh or frames_changed[r] for r in range(R)]
    flagged = []
    for r in range(R):
        flag = listed[r].copy()                                              # a rebuilt slot: its rows, so its span, may differ
        k = 0 if first else old_sub[r]
        if whole[r]:
            flag[:] = True
        elif k and n_frames[r] > old_nf[r]:                                  # an old slot gains a candidate only when an appended frame's time lies in its span
            ta = np.asarray(frames[r].times, dtype=np.float64).reshape(-1)[old_nf[r]:]
            sp = state.span_h[int(old_sub_off[r]):int(old_sub_off[r]) + k]
            flag[:k] |= ((ta[None, :] >= sp[:, :1]) & (ta[None, :] <= sp[:, 1:])).any(axis=1)
        flagged.append(flag)
    flst = np.concatenate([int(sub_off[r]) + np.nonzero(f)[0] for r, f in enumerate(flagged)]).astype(np.int32)
    # capacity: the frame tensors as the session's other tensors; a mask row's words grow when ceil(Nf_r / 64) exceeds them
    words = [(n + 63) // 64 for n in n_frames]
    mw = [m if w <= m else int(np.ceil(w * GROWTH)) for w, m in zip(words, old_mw)]
    off = lambda n: [int(x) for x in np.concatenate([[0], np.cumsum(n)])]
    frame_off, old_frame_off = off(n_frames), off(old_nf)
    k_old = [0] * R if (first or fresh) else list(old_sub)
    mask_off, old_mask_off = off([k * w for k, w in zip(n_sub, mw)]), off([k * w for k, w in zip(k_old, old_mw)])
    S, NF = int(sub_off[-1]), frame_off[-1]
    shapes = dict(f_times=((), torch.float64), f_pos=((3,), torch.float64), f_desc=((d,), torch.float64), f_n=((), torch.int32), f_span=((2,), torch.float64))
    for name, (per, unit, fill) in _SESSION_FRAME_TENSORS.items():
        if fresh:
            t[name] = torch.full((0,) + shapes[name][0], fill, dtype=shapes[name][1], device=dev)
        o_off, n_off, o_len, total = (old_frame_off, frame_off, old_nf, max(NF, 1)) if unit == 'frm' else ([int(x) for x in old_sub_off], [int(x) for x in sub_off], k_old, max(S, 1))
        t[name] = _moved(torch, t[name], o_off[:-1], o_len, n_off[:-1], total, per, fill)
    if fresh:
        t["f_mask"] = torch.zeros((0,), dtype=torch.int64, device=dev)
    t["f_mask"] = _moved_mask(torch, t["f_mask"], old_mask_off[:-1], k_old, old_mw, mask_off[:-1], mw, max(mask_off[-1], 1))
    uploaded = 0
    for r, fr in enumerate(frames):
        a = 0 if whole[r] else old_nf[r]
        if n_frames[r] > a:
            lo = frame_off[r]
            for name, arr in (("f_times", fr.times.reshape(-1)), ("f_pos", fr.pos.reshape(-1, 3)), ("f_desc", fr.desc.reshape(n_frames[r], -1))):
                t[name][lo + a:lo + n_frames[r]].copy_(torch.from_numpy(np.ascontiguousarray(arr[a:], dtype=np.float64)))
            uploaded += n_frames[r] - a
    ft = []
    for r in range(R):
        lo, hi = int(sub_off[r]), int(sub_off[r + 1])
        ft.append(dict(W=words[r], n=t["f_n"][lo:hi], mask=t["f_mask"][mask_off[r]:mask_off[r + 1]].view(hi - lo, mw[r]),
                       desc=t["f_desc"][frame_off[r]:frame_off[r + 1]]))
    robots = session_frame_robots(n_rows, n_sub, n_frames, mw)
    return ft, flst, robots, torch.zeros(max(len(flst), 1), dtype=torch.int32, device=dev), mw, uploaded


def _moved_mask(torch, t, old_off, old_sub, old_words, new_off, new_words, total):
    """The mask words `t` with robot r's old_sub[r] rows of old_words[r] words moved from word old_off[r] to new_off[r] and laid out
    in rows of new_words[r] >= old_words[r] words: `_moved` while every robot keeps its row length; else into a tensor GROWTH times
    the need, old rows copied to the new stride on the device, new words zero."""
    if list(old_words) == list(new_words):
        return _moved(torch, t, old_off, [k * w for k, w in zip(old_sub, old_words)], new_off, total, 1, 0)
    new = torch.zeros((max(int(total * GROWTH), 1),), dtype=t.dtype, device=t.device)
    for o, n, k, wo, wn in zip(old_off, new_off, old_sub, old_words, new_words):
        if k and wo:
            new[n:n + k * wn].view(k, wn)[:, :wo].copy_(t[o:o + k * wo].view(k, wo))
    return new


def grow_session_pools(state, registration, tables, centers, params, ctx=None, device=None, cap=None, frames=None, changed_rows=None, rebuild=None,
                       frames_changed=None):
    """build_session_pools for a session that GROWS -> (pools, touched, state).  `state` (a SessionPoolsState, or
    None before the first call) keeps the session's tables and pools in HBM; a call uploads only the appended and the rewritten
    table rows, rebuilds only the submaps that are new or can have changed — ONE roman_session_submaps_list_dev call, one
    synchronisation, one read-back of the small arrays — and learns from the device which slots really changed.  The pools equal,
    field by field and byte for byte, build_session_pools(registration, tables, centers, params, cap=<the state's cap>) over the same
    inputs, views of one storage in robot order; touched[r] (bool per submap of robot r) is the `touched` argument of
    submap_align_session_update: the new submaps and the rebuilt old ones of which a byte changed (in the frame-descriptor modes
    also those whose frame mask, frame count or mean changed).  The pools of an earlier step are views of the same storage: they are
    not to be read after the next call.

    Between two calls a table may grow by APPENDED rows (found from the lengths) and have rows rewritten in place, which the caller
    names in changed_rows[r] (indices, or None); centres may only be appended, an old centre's record may change (t_hi of the former
    last submap does).  Rebuilt are: every new submap; every old one whose roman_submap_desc_t bytes differ from the recorded ones;
    every old submap s of robot r for which an appended or named row k was a member (k in src[s, :count[s]]) or passes the time window
    with its new times, NOT (first_seen > t_hi[s] OR last_seen < t_lo[s]); and whatever rebuild[r] names (rebuild='all': everything).

    The frame-descriptor modes over a context with session_frame_select_list_dev: the frame tables stay in HBM
    too.  A frame table may only grow by APPENDED frames (found from the lengths; only they go up) unless frames_changed[r] (one
    bool per robot, default none) says that robot r's table was rewritten: it goes up whole and all its submaps are reselected.
    ONE session_frame_select_list_dev call behind the rebuild reselects the rebuilt submaps, every old one whose recorded span
    holds an appended frame's time, and those of a frames_changed robot; `touched` is the union of what the two calls report as
    changed.  pool.frame_mask and pool.frame_desc_dev are strided views of the session's tensors.  state.frames_uploaded and
    state.frames_listed count what the call moved and reselected.  A context without that entry reselects per robot as
    build_session_pools does.

    ValueError before a context is made: whatever build_session_pools refuses (the force-fill mode included); a robot count, cap,
    row layout or submap_descriptor other than the state's; a table, centre list or frame table that shrank; changed_rows out of
    range; a frames_changed that does not hold one entry per robot; a state whose last call raised after it had begun to move the
    session's tensors (state.unfinished: the new layout is recorded in one place, at the end of a call).  ValueError with the
    context, before anything moves: a state with resident frame tables and a context without session_frame_select_list_dev."""
    import time
    import torch
    marks = [time.perf_counter()]
    tables, centers, frames, P, (d, framed, mean_frames) = _session_refusals(tables, centers, params, cap, frames, None)
    R = len(tables)
    state = SessionPoolsState() if state is None else state
    layout = None if R == 0 else (int(tables[0].feats.shape[1]), int(tables[0].point_dim), int(tables[0].desc_dim), tables[0].invariant)
    key = (R, None if P is None else int(P.cap), layout, params.submap_descriptor, int(d))
    if state.unfinished:
        raise ValueError("the state's last call raised after it had begun to move the session's tensors: they no longer match what the "
                         "state records, begin again with a new state")
    if state.key is not None and state.key != key:
        raise ValueError("the state was made for another robot count, cap, row layout or submap_descriptor: a SessionPoolsState serves one session")
    first = state.key is None
    old_rows, old_sub = ([0] * R, [0] * R) if first else (state.n_rows, state.n_sub)
    n_rows, n_sub = [len(t) for t in tables], [len(c) for c in centers]
    if any(n < m for n, m in zip(n_rows, old_rows)) or any(n < m for n, m in zip(n_sub, old_sub)):
        raise ValueError("a table or a centre list shrank: between two calls rows and centres may only be appended")
    changed_rows = [None] * R if changed_rows is None else list(changed_rows)
    if len(changed_rows) != R:
        raise ValueError("changed_rows must hold one entry per table, each None or the indices of the rewritten rows")
    named = []
    for r, rows in enumerate(changed_rows):
        rows = np.zeros(0, dtype=np.int64) if rows is None else np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
        if len(rows) and (rows[0] < 0 or rows[-1] >= n_rows[r]):
            raise ValueError(f"changed_rows[{r}] names a row outside the table's {n_rows[r]} rows")
        named.append(rows[rows < old_rows[r]])                               # (a named row beyond the old length is an appended one)
    if not (rebuild is None or isinstance(rebuild, str) and rebuild == 'all'):
        rebuild = list(rebuild)
        if len(rebuild) != R or any(x is not None and len(np.asarray(x).reshape(-1)) and
                                    (np.min(x) < 0 or np.max(x) >= n) for x, n in zip(rebuild, n_sub)):
            raise ValueError("rebuild must be None, 'all', or one entry per robot, each None or submap indices of that robot")
    frames_changed = [False] * R if frames_changed is None else [bool(x) for x in frames_changed]
    if len(frames_changed) != R:
        raise ValueError("frames_changed must hold one bool per table")
    n_frames = [len(f) for f in frames] if framed else [0] * R
    if framed and state.n_frames is not None and any(n < m for n, m in zip(n_frames, state.n_frames)):
        raise ValueError("a frame table shrank: between two calls frames may only be appended")
    if R == 0:
        return [], [], state

    # ---- the list: every rule is a necessary condition for a slot to change, so what is left out cannot have ----
    seg_off = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum(n_sub)]).astype(np.int32)
    old_seg_off, old_sub_off = np.concatenate([[0], np.cumsum(old_rows)]).astype(np.int64), np.concatenate([[0], np.cumsum(old_sub)]).astype(np.int64)
    descs_r = [c.descs() for c in centers]
    desc_bytes = [np.ascontiguousarray(x).view(np.uint8).reshape(len(x), x.dtype.itemsize).copy() for x in descs_r]       # (a robot without submaps: (0, bytes))
    listed = []
    for r in range(R):
        flag = np.zeros(n_sub[r], dtype=bool)
        flag[old_sub[r]:] = True
        k_old = old_sub[r]
        if rebuild is not None:
            if isinstance(rebuild, str):
                flag[:] = True
            elif rebuild[r] is not None:
                flag[np.asarray(rebuild[r], dtype=np.int64).reshape(-1)] = True
        if k_old:
            flag[:k_old] |= (desc_bytes[r][:k_old] != state.descs[r]).any(axis=1)
            rows = np.concatenate([named[r], np.arange(old_rows[r], n_rows[r], dtype=np.int64)])
            if len(rows):
                tm = np.asarray(tables[r].times, dtype=np.float64).reshape(-1, 2)[rows]
                dd = descs_r[r][:k_old]
                flag[:k_old] |= (~((tm[None, :, 0] > dd["t_hi"][:, None]) | (tm[None, :, 1] < dd["t_lo"][:, None]))).any(axis=1)
                if len(named[r]):
                    lo = int(old_sub_off[r])
                    src_r, cnt_r = state.src_h[lo:lo + k_old], state.count_h[lo:lo + k_old]
                    member = np.isin(src_r, named[r]) & (np.arange(src_r.shape[1])[None, :] < cnt_r[:, None])
                    flag[:k_old] |= member.any(axis=1)
        listed.append(flag)
    lst = np.concatenate([int(sub_off[r]) + np.nonzero(f)[0] for r, f in enumerate(listed)]).astype(np.int32)

    # ---- the device: capacity, every robot's range next to the one in front of it, the new table rows ----
    ctx = ctx or registration._context()
    dev = torch.device(device if device is not None else f"cuda:{getattr(ctx, 'device', 0)}")
    on_host = dev.type == "cpu"                                              # CPU tensors + a stand-in context (tests)
    resident = framed and hasattr(ctx, "session_frame_select_list_dev")     # the frame tables stay in HBM too
    if framed and not resident and state.n_frames is not None:
        raise ValueError("the state keeps the session's frame tables on the device (DESIGN.md §4.23) and this context has no "
                         "session_frame_select_list_dev: a session stays with the kind of context it began with")
    state.unfinished = True                                                  # from here the session's tensors move; cleared when the new layout is recorded
    F, capn = layout[0], int(P.cap)
    Fo, S, N = P.point_dim + F - 3, int(sub_off[-1]), int(seg_off[-1])
    shapes = dict(feats=((F,), torch.float64), times=((2,), torch.float64), ids=((), torch.int64), pool=((Fo,), torch.float64), src=((), torch.int32),
                  ids_out=((), torch.int64), count=((), torch.int32), status=((), torch.int32), desc=((max(d, 1),), torch.float64))
    t = state.t
    for name, (per, unit, fill) in _SESSION_TENSORS.items():
        per = capn if per == 'cap' else 1
        if first:
            t[name] = torch.full((0,) + shapes[name][0], fill, dtype=shapes[name][1], device=dev)
        o_off, n_off, o_len, total = (old_seg_off, seg_off, old_rows, max(N, 1)) if unit == 'seg' else (old_sub_off, sub_off, old_sub, max(S, 1))
        t[name] = _moved(torch, t[name], [int(x) for x in o_off[:-1]], o_len, [int(x) for x in n_off[:-1]], total, per, fill)
        if unit == 'sub':                                                    # a new slot starts as a fresh build's does
            for r in range(R):
                t[name][(int(sub_off[r]) + old_sub[r]) * per:int(sub_off[r + 1]) * per] = fill
    for r, tb in enumerate(tables):
        lo = int(seg_off[r])
        for name, a, dt in (("feats", tb.feats, np.float64), ("times", tb.times.reshape(-1, 2), np.float64), ("ids", tb.ids.reshape(-1), np.int64)):
            if n_rows[r] > old_rows[r]:
                t[name][lo + old_rows[r]:lo + n_rows[r]].copy_(torch.from_numpy(np.ascontiguousarray(a[old_rows[r]:], dtype=dt)))
            if len(named[r]):
                t[name][torch.from_numpy(named[r] + lo).to(dev)] = torch.from_numpy(np.ascontiguousarray(a[named[r]], dtype=dt)).to(dev)
    changed = torch.zeros(max(len(lst), 1), dtype=torch.int32, device=dev)
    ft, before, flst = [], None, lst
    if resident:
        ft, flst, robots, fchanged, mask_words, uploaded = _grow_frames(torch, dev, state, frames, frames_changed, first, listed, n_rows, n_sub, old_sub, n_frames, sub_off,
                                                  old_sub_off)
    elif framed:
        ft = _frame_tensors(torch, dev, frames, centers)
        before = [None if first or not old_sub[r] else dict(state.frame[r], mean=t["desc"][int(sub_off[r]):int(sub_off[r]) + old_sub[r]].clone())
                  for r in range(R)]
        if mean_frames:                                                      # frame_select_dev writes the mean of every non-empty submap again and leaves
            t["desc"][:S] = float("nan")                                     # an empty one's row alone: NaN there, as in a fresh build
    if not on_host:
        torch.cuda.current_stream(dev).synchronize()                         # moves, uploads and cleared slots are in place before the library's stream touches them
    marks.append(time.perf_counter())
    descs = np.concatenate(descs_r)
    ctx.session_submaps_list_dev(P, F, seg_off, t["feats"].data_ptr(), t["times"].data_ptr(), sub_off, descs, lst, t["pool"].data_ptr(), t["count"].data_ptr(),
                                 t["src"].data_ptr(), t["status"].data_ptr(), seg_ids_ptr=t["ids"].data_ptr(), ids_out_ptr=t["ids_out"].data_ptr() if N else None,
                                 desc_dim=0 if framed else d, desc_out_ptr=t["desc"].data_ptr() if d and not framed else None,
                                 changed_ptr=changed.data_ptr())
    if resident:                                                             # ONE call behind it on the same stream: it reads the count and src of the slots just rebuilt
        thin = params.frame_descriptor_dist if params.submap_descriptor == 'stacked_frame_descriptors' else None      # [REF roman/map/map.py:216-226]
        ctx.session_frame_select_list_dev(frame_select_params(thin, mean_frames), robots, capn, t["count"].data_ptr(), t["src"].data_ptr(), t["times"].data_ptr(),
                                          t["f_times"].data_ptr(), flst, t["f_mask"].data_ptr(), t["f_n"].data_ptr(), t["f_span"].data_ptr(), fchanged.data_ptr(),
                                          frame_pos_ptr=t["f_pos"].data_ptr(), d=int(t["f_desc"].shape[1]), frame_desc_ptr=t["f_desc"].data_ptr(),
                                          mean_ptr=t["desc"].data_ptr() if mean_frames else None)
    elif framed:                                                             # behind it on the same stream, over every submap of a robot as in build_session_pools
        _frame_select_robots(ctx, params, P, tables, frames, seg_off, sub_off, mean_frames, t["count"], t["src"], t["times"], t["desc"], ft)
    ctx.sync()
    marks.append(time.perf_counter())

    # ---- one read-back of the small arrays ----
    rows = S * capn
    count_h, status_h = t["count"].cpu().numpy()[:S].copy(), t["status"].cpu().numpy()[:S].copy()
    src_h, ids_h = t["src"].cpu().numpy()[:rows].reshape(S, capn).copy(), t["ids_out"].cpu().numpy()[:rows].reshape(S, capn).copy()
    desc_h = t["desc"].cpu().numpy()[:S, :d] if d else None
    changed_h = changed.cpu().numpy()[:len(lst)]
    differs_h = np.zeros(S, dtype=bool)                                      # by global slot: what the device reports as changed
    differs_h[lst[changed_h != 0]] = True
    if resident:
        differs_h[flst[fchanged.cpu().numpy()[:len(flst)] != 0]] = True
        span_h, fn_h = t["f_span"][:S].cpu().numpy(), t["f_n"][:S].cpu().numpy()
        for r in range(R):                                                   # (read back once, sliced on the host)
            ft[r]["n_h"] = fn_h[int(sub_off[r]):int(sub_off[r + 1])]
    touched = []
    for r in range(R):
        flag = differs_h[int(sub_off[r]):int(sub_off[r + 1])].copy()
        flag[old_sub[r]:] = True
        if before is not None and before[r] is not None:                                 # what frame_select_dev left for the old submaps against the last call's, on the device
            k, f, b = old_sub[r], ft[r], before[r]
            W = max(int(f["mask"].shape[1]), int(b["mask"].shape[1]))
            wide = lambda m: torch.nn.functional.pad(m[:k], (0, W - int(m.shape[1])))
            differs = (wide(f["mask"]) != wide(b["mask"])).any(dim=1) | (f["n"][:k] != b["n"][:k])
            if mean_frames:
                now = t["desc"][int(sub_off[r]):int(sub_off[r]) + k]
                differs |= (now.contiguous().view(torch.int64) != b["mean"].contiguous().view(torch.int64)).any(dim=1)
            flag[:k] |= differs.cpu().numpy()
        touched.append(flag)
    pools = _session_pool_views(tables, centers, frames, params, P, sub_off, d, framed, t["pool"], t["ids_out"], t["desc"], count_h, status_h, src_h, ids_h,
                                desc_h, ft)
    state.key, state.n_rows, state.n_sub, state.descs = key, n_rows, n_sub, desc_bytes
    state.count_h, state.src_h = count_h, src_h
    state.frame = [dict(mask=f["mask"], n=f["n"]) for f in ft] if framed and not resident else None
    state.listed, state.total = int(len(lst)), S
    state.frames_listed = int(len(flst)) if resident else (S if framed else 0)
    if resident:
        state.n_frames, state.mask_words, state.frames_uploaded, state.span_h = list(n_frames), mask_words, uploaded, span_h
    state.unfinished = False
    marks.append(time.perf_counter())
    state.seconds = dict(upload=marks[1] - marks[0], device=marks[2] - marks[1], readback=marks[3] - marks[2])
    return pools, touched, state
