"""Segment update on the device.

With every pair the Hungarian solve returns, the reference's mapper calls `Segment.update` [REF roman/object/segment.py:100-120]:
the observation's cloud is transformed into the world frame, appended to the segment's and cleaned by open3d
(`voxel_down_sample`, then `remove_statistical_outlier(10, std)`: a 10-nearest-neighbour search for every point)
[REF roman/object/segment.py:133-193].  Every new segment [REF :98] and every merge [REF :122-161] run the same clean-up.  Here
the clouds of both sides are ONE array each (`SegmentClouds`), a frame's updates are a LIST OF JOBS, and one device call
(roman_segment_integrate) writes every job's cleaned cloud.  The descriptor's running mean (`_add_semantic_descriptor`
[REF :474-489], d flops per job) stays on the host, below.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..align.segment_clouds import SegmentClouds
from ..runtime import cluster_params, integrate_jobs, integrate_params
from .association import _clouds


@dataclass
class IntegrationParams:
    """The fields of MapperParams the update reads [REF roman/params/mapper_params.py:73-74], under the same names."""
    segment_voxel_size: float = 0.05
    segment_outlier_removal_std: Optional[float] = 1.0     # None, <= 0 or infinite: no outlier removal [REF :100-103]

    @classmethod
    def from_mapper_params(cls, p):
        """Reads the reference's field names off a MapperParams-like object."""
        return cls(float(p.segment_voxel_size), p.segment_outlier_removal_std)

    def abi(self):
        """-> roman_integrate_params_t.  Everything the C ABI would refuse is a ValueError here, before any context exists."""
        vs = float(self.segment_voxel_size)
        if not (np.isfinite(vs) and vs > 0):
            raise ValueError(f"segment_voxel_size must be finite and > 0 (got {vs})")
        std = self.segment_outlier_removal_std
        if std is not None and np.isnan(float(std)):
            raise ValueError("segment_outlier_removal_std is NaN")
        return integrate_params(vs, std)


@dataclass
class IntegrationResult:
    """clouds: the cleaned clouds in job order (a job that ends without points holds none: the reference's points = None);
    status (n_jobs,) ROMAN_ASSOC_OK / _EMPTY / _RANGE; threshold (n_jobs,): the outlier step's distance threshold, NaN for a job
    that did not run it; desc_counts (n_jobs,): observations behind every descriptor (semantic_descriptor_cnt)."""
    clouds: SegmentClouds
    status: np.ndarray
    threshold: np.ndarray
    desc_counts: np.ndarray


def _descriptor(base, cnt_base, add, cnt_add):
    """_add_semantic_descriptor [REF roman/object/segment.py:474-489] in its operation order: the first descriptor over its norm,
    or the running mean; then, in both cases, the result over its own norm (the reference's renormalisation, :489)."""
    if base is None:
        d = add / np.linalg.norm(add)
    else:
        d = base * cnt_base / (cnt_base + cnt_add) + add * cnt_add / np.linalg.norm(add) / (cnt_base + cnt_add)
    return d / np.linalg.norm(d)


def _prepared(segments, added, jobs, params, poses, segment_counts, added_counts):
    """What integrate refuses before any context is made -> (iparams, points, cloud_off, job table, poses, segment side, added side)."""
    iparams = params.abi()
    ps, os_, ds = _clouds(segments, "segments")
    pa, oa, da = _clouds(added, "added")
    ns, na = len(os_) - 1, len(oa) - 1
    table = integrate_jobs(jobs)
    if poses is not None:
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (4, 4):
            raise ValueError(f"poses must be (n_poses, 4, 4) (got {poses.shape})")
    n_poses = 0 if poses is None else len(poses)
    seen = set()
    for k, j in enumerate(table):
        if not -1 <= j["base"] < ns:
            raise ValueError(f"job {k}: base = {j['base']} is neither None nor one of the {ns} segments")
        if not 0 <= j["add"] < na:
            raise ValueError(f"job {k}: add = {j['add']} is not one of the {na} added clouds")
        if not -1 <= j["pose"] < n_poses:
            raise ValueError(f"job {k}: pose = {j['pose']} is neither None nor one of the {n_poses} poses")
        if j["base"] >= 0 and int(j["base"]) in seen:
            raise ValueError(f"job {k}: segment {j['base']} is the base of an earlier job")
        seen.add(int(j["base"]))
    if ds is not None and da is not None and ds.shape[1] != da.shape[1]:
        raise ValueError(f"the descriptors of the two sides differ in width ({ds.shape[1]}, {da.shape[1]})")
    cs = np.ones(ns, dtype=np.int64) if segment_counts is None else np.asarray(segment_counts, dtype=np.int64).reshape(-1)
    ca = np.ones(na, dtype=np.int64) if added_counts is None else np.asarray(added_counts, dtype=np.int64).reshape(-1)
    if cs.shape[0] != ns or ca.shape[0] != na:
        raise ValueError("segment_counts / added_counts must hold one count per cloud")
    table = table.copy()
    table["add"] += ns                                        # the added clouds stand behind the segments' in the call's one array
    return (iparams, np.ascontiguousarray(np.vstack([ps, pa])), np.concatenate([os_, os_[-1] + oa[1:]]), table, poses,
            (segments, ds, cs), (added, da, ca), ns)


def integrate(segments, added, jobs, params, poses=None, ctx=None, segment_counts=None, added_counts=None) -> IntegrationResult:
    """A frame's segment updates in one call.  `segments` and `added` are SegmentClouds; a job is (base, add) or (base, add, pose):
    base an index into `segments` or None for a new segment, add an index into `added`, pose an index into `poses` (n_poses, 4, 4)
    or None when the added cloud is in the world frame already (a merge; SegmentClouds.from_observations).  A segment is the base
    of at most one job.  -> IntegrationResult; ids and first_seen come from the base or, for a new segment, from the added cloud,
    last_seen is the later of the two [REF roman/object/segment.py:118-119], and where both sides carry descriptors the running
    mean of _add_semantic_descriptor, renormalised as there, is applied with the counts given (default 1 each)."""
    iparams, points, off, table, poses, (S, ds, cs), (A, da, ca), ns = _prepared(segments, added, jobs, params, poses, segment_counts, added_counts)
    n_jobs = len(table)
    if n_jobs == 0:
        d = None if (ds is None or da is None) else np.zeros((0, ds.shape[1]))
        return IntegrationResult(SegmentClouds(np.zeros((0, 3)), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), d),
                                 np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int64))
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    out = ctx.segment_integrate(iparams, points, off, table, poses)
    seg_off = np.concatenate([[0], np.cumsum(out.count, dtype=np.int64)]).astype(np.int64)
    cloud = np.ascontiguousarray(np.vstack([out.cloud(j) for j in range(n_jobs)]))
    ids, times, counts = np.zeros(n_jobs, np.int64), np.zeros((n_jobs, 2)), np.zeros(n_jobs, np.int64)
    desc = None if (ds is None or da is None) else np.zeros((n_jobs, ds.shape[1]))
    for k, j in enumerate(table):
        b, a = int(j["base"]), int(j["add"]) - ns
        src, i = (S, b) if b >= 0 else (A, a)
        ids[k] = np.asarray(src.ids)[i]
        times[k, 0] = np.asarray(src.times)[i, 0]
        times[k, 1] = max(np.asarray(src.times)[i, 1], np.asarray(A.times)[a, 1])
        counts[k] = (cs[b] if b >= 0 else 0) + ca[a]
        if desc is not None:
            desc[k] = _descriptor(ds[b] if b >= 0 else None, cs[b] if b >= 0 else 0, da[a], ca[a])
    return IntegrationResult(SegmentClouds(cloud, seg_off, ids, times, desc), out.status, out.thr, counts)


def cleanup_points(points, params, ctx=None):
    """What Segment._cleanup_points does to a cloud [REF roman/object/segment.py:177-193]: one job without a base -> (count, 3);
    no row is the reference's points = None."""
    iparams = params.abi()
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (n, 3) (got {points.shape})")
    if len(points) == 0:
        return np.zeros((0, 3))
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    out = ctx.segment_integrate(iparams, points, np.array([0, len(points)], dtype=np.int64), [(None, 0, None)])
    return out.cloud(0).copy()


# ------------------------------------------------------------------------------------------------ segment clustering
@dataclass
class ClusterParams:
    """What Mapper.update hands to Segment.final_cleanup [REF roman/map/mapper.py:101]: MapperParams.clustering_epsilon
    [REF roman/params/mapper_params.py:68] and final_cleanup's own min_points [REF roman/object/segment.py:195]."""
    clustering_epsilon: float = 0.25
    min_points: int = 10

    @classmethod
    def from_mapper_params(cls, p, min_points=10):
        """Reads the reference's field name off a MapperParams-like object."""
        return cls(float(p.clustering_epsilon), int(min_points))

    def abi(self):
        """-> roman_cluster_params_t.  Everything the C ABI would refuse is a ValueError here, before any context exists."""
        eps = float(self.clustering_epsilon)
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError(f"clustering_epsilon must be finite and > 0 (got {eps})")
        if int(self.min_points) != self.min_points or int(self.min_points) < 1:
            raise ValueError(f"min_points must be an integer >= 1 (got {self.min_points})")
        return cluster_params(eps, int(self.min_points))


@dataclass
class CleanupResult:
    """clouds: the kept clusters in `which` order (a dropped segment holds no point); dropped: the subset of `which` without a
    cluster or without points — the mapper's except branch and its num_points == 0 branch [REF roman/map/mapper.py:97-105];
    status, n_clusters, kept (len(which),): what roman_segment_cluster wrote."""
    clouds: SegmentClouds
    dropped: np.ndarray
    status: np.ndarray
    n_clusters: np.ndarray
    kept: np.ndarray


def _subset(segments, which, points, off):
    desc = None if segments.descriptors is None else np.ascontiguousarray(np.asarray(segments.descriptors)[which])
    return SegmentClouds(points, off, np.asarray(segments.ids)[which].astype(np.int64), np.asarray(segments.times, dtype=np.float64).reshape(-1, 2)[which], desc)


def final_cleanup(segments, which, params, ctx=None) -> CleanupResult:
    """Segment.final_cleanup [REF roman/object/segment.py:195-220] for the segments `which` (indices into `segments`, each at most
    once) in one device call.  -> CleanupResult; ids, times and descriptors are carried over unchanged."""
    cparams = params.abi()
    points, off, _ = _clouds(segments, "segments")
    which = np.asarray(which, dtype=np.int64).reshape(-1)
    n = len(off) - 1
    if len(which) and (which.min() < 0 or which.max() >= n):
        raise ValueError(f"which names a segment outside the {n} given")
    if len(np.unique(which)) != len(which):
        raise ValueError("which names a segment twice")
    if len(which) == 0:
        z = np.zeros(0, np.int32)
        return CleanupResult(_subset(segments, which, np.zeros((0, 3)), np.zeros(1, np.int64)), np.zeros(0, np.int64), z, z.copy(), z.copy())
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    out = ctx.segment_cluster(cparams, points, off, which, want_labels=False)
    kept_off = np.concatenate([[0], np.cumsum(out.count, dtype=np.int64)]).astype(np.int64)
    cloud = np.ascontiguousarray(np.vstack([out.cloud(j) for j in range(len(which))]))
    return CleanupResult(_subset(segments, which, cloud, kept_off), which[out.count == 0], out.status, out.n_clusters, out.kept)


def cluster_labels(points, params, ctx=None):
    """open3d's cluster_dbscan labels of one cloud (n,) int32, -1: noise — as roman_segment_cluster restates them."""
    cparams = params.abi()
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (n, 3) (got {points.shape})")
    if len(points) == 0:
        return np.zeros(0, np.int32)
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    return ctx.segment_cluster(cparams, points, np.array([0, len(points)], dtype=np.int64), [0]).labels(0).copy()


def retire(segments, t, last_seen, max_t_no_sightings, params, ctx=None):
    """The mapper's move to inactive [REF roman/map/mapper.py:92-105]: the segments with t - last_seen > max_t_no_sightings, or
    without points, leave `segments`; those with points go through final_cleanup.  last_seen (N,) or None for segments.times[:, 1].
    -> (indices that stay active, the inactive SegmentClouds, the ids that were dropped — no points, or no cluster)."""
    _, off, _ = _clouds(segments, "segments")
    n = len(off) - 1
    seen = np.asarray(segments.times, dtype=np.float64).reshape(-1, 2)[:, 1] if last_seen is None else np.asarray(last_seen, dtype=np.float64).reshape(-1)
    if seen.shape[0] != n:
        raise ValueError(f"last_seen must hold one time per segment ({n})")
    empty = np.diff(off) == 0
    leave = (float(t) - seen > float(max_t_no_sightings)) | empty
    res = final_cleanup(segments, np.flatnonzero(leave & ~empty), params, ctx=ctx)
    alive = np.diff(res.clouds.seg_off) > 0
    inactive = _subset(res.clouds, np.flatnonzero(alive), res.clouds.points, np.concatenate([[0], np.cumsum(np.diff(res.clouds.seg_off)[alive])]).astype(np.int64))
    dropped = np.concatenate([np.asarray(segments.ids)[np.flatnonzero(empty)], np.asarray(res.clouds.ids)[~alive]]).astype(np.int64)
    return np.flatnonzero(~leave), inactive, dropped
