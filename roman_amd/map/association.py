"""Frame data association on the device.

Every frame the reference's mapper calls `global_nearest_neighbor(segments + nursery, observations, similarity_function,
similarity_range)` [REF roman/map/mapper.py:65-68]: a Python loop over all pairs that voxelises both clouds with open3d and
intersects two dense arrays (`VoxelGrid.iou` [REF roman/map/voxel_grid.py:32-83]), then a Hungarian solve; `merge()` calls the
same similarity for every pair of segments [REF roman/map/mapper.py:276-299].  Here the clouds of either side are ONE array
(`SegmentClouds`), one device call (roman_assoc_scores_dev) writes the similarity and score matrices, and the Hungarian solve
over the augmented cost matrix stays on the host — it is small and sequential.  Results come back as NumPy arrays, so the
host-pointer form of the call carries the clouds up and the matrices back; a caller that keeps its clouds on the device uses
Context.assoc_scores_dev.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _abi
from ..runtime import AssocScores, assoc_params

_NOT_COVERED = "geometric_association_method='chamfer' is not covered (DESIGN.md §4.25, Not covered): use 'iou' or 'iom'"


@dataclass
class AssociationParams:
    """The fields of MapperParams the association reads [REF roman/params/mapper_params.py:58-72], under the same names."""
    geometric_association_method: str = "iou"
    semantic_association_method: Optional[str] = None          # None / 'none' / 'cosine_similarity'
    geometric_score_range: Tuple[float, float] = (0.25, 1.0)
    semantic_score_range: Tuple[float, float] = (0.8, 1.0)
    iou_voxel_size: float = 0.2

    @classmethod
    def from_mapper_params(cls, p):
        """Reads the reference's field names off a MapperParams-like object."""
        return cls(p.geometric_association_method, p.semantic_association_method, tuple(p.geometric_score_range),
                   tuple(p.semantic_score_range), float(p.iou_voxel_size))

    @property
    def semantic(self) -> bool:
        m = self.semantic_association_method
        return m is not None and str(m).lower() != "none"

    def abi(self):
        """-> roman_assoc_params_t.  Everything the C ABI would refuse is a ValueError here, before any context exists."""
        g = self.geometric_association_method
        if g == "chamfer":
            raise ValueError(_NOT_COVERED)
        if g not in _abi.ASSOC_GEOMETRIC:
            raise ValueError(f"geometric_association_method must be one of {sorted(_abi.ASSOC_GEOMETRIC)} (got {g!r})")
        if self.semantic and self.semantic_association_method != "cosine_similarity":
            raise ValueError(f"semantic_association_method must be None, 'none' or 'cosine_similarity' (got {self.semantic_association_method!r})")
        vs = float(self.iou_voxel_size)
        if not (np.isfinite(vs) and vs > 0):
            raise ValueError(f"iou_voxel_size must be finite and > 0 (got {vs})")
        for name, r, used in (("geometric_score_range", self.geometric_score_range, True), ("semantic_score_range", self.semantic_score_range, self.semantic)):
            if len(r) != 2:
                raise ValueError(f"{name} must be (threshold, maximum)")
            if used and (np.isnan(float(r[0])) or not float(r[1]) != float(r[0])):
                raise ValueError(f"{name} = {tuple(r)}: threshold and maximum must differ")
        return assoc_params(vs, g, self.semantic, self.geometric_score_range, self.semantic_score_range)


def _clouds(c, what):
    """The arrays of a SegmentClouds, checked -> (points (P, 3), off (N + 1,), descriptors (N, d) or None)."""
    try:
        points = np.ascontiguousarray(c.points, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: points must be convertible to float64: {e}") from None
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (P, 3) (got {points.shape})")
    off = np.ascontiguousarray(c.seg_off, dtype=np.int64).reshape(-1)
    if off.shape[0] < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or int(off[-1]) != points.shape[0]:
        raise ValueError(f"{what}: seg_off must ascend from 0 to the number of points")
    desc = None if c.descriptors is None else np.ascontiguousarray(c.descriptors, dtype=np.float64)
    if desc is not None and (desc.ndim != 2 or desc.shape[0] != off.shape[0] - 1):
        raise ValueError(f"{what}: descriptors must be (N, d)")
    return points, off, desc


def _stacked(clouds_a, clouds_b, params):
    """What association_scores refuses before any context is made -> (aparams, points, cloud_off, N1, N2, desc or None)."""
    aparams = params.abi()
    pa, oa, da = _clouds(clouds_a, "clouds_a")
    if clouds_b is None:
        return aparams, pa, oa, len(oa) - 1, -1, (da if aparams.semantic else None)
    pb, ob, db = _clouds(clouds_b, "clouds_b")
    desc = None
    if aparams.semantic and da is not None and db is not None:          # a side without descriptors: the cosine is 1.0 [REF roman/map/mapper.py:208-209]
        if da.shape[1] != db.shape[1]:
            raise ValueError(f"the descriptors of the two sides differ in width ({da.shape[1]}, {db.shape[1]})")
        desc = np.ascontiguousarray(np.vstack([da, db]))
    return aparams, np.ascontiguousarray(np.vstack([pa, pb])), np.concatenate([oa, oa[-1] + ob[1:]]), len(oa) - 1, len(ob) - 1, desc


def association_scores(clouds_a, clouds_b, params, ctx=None) -> AssocScores:
    """The similarity and score matrices of global_nearest_neighbor's pair loop [REF roman/map/global_nearest_neighbor.py:23-36]:
    rows are the clouds of `clouds_a` (a frame's segments and nursery), columns those of `clouds_b` (its observations), both
    SegmentClouds; clouds_b None: self mode, as merge() compares segments.  -> AssocScores of NumPy arrays: geo, sem (None without
    a semantic method), score, inter (N1, N2); n_vox, status per cloud, rows first."""
    aparams, points, off, N1, N2, desc = _stacked(clouds_a, clouds_b, params)
    cols = N1 if N2 < 0 else N2
    clouds = len(off) - 1
    if N1 == 0 or cols == 0:
        z = np.zeros((N1, cols))
        return AssocScores(z, z.copy() if aparams.semantic else None, z.copy(), np.zeros(clouds, np.int32), np.zeros((N1, cols), np.int32), np.zeros(clouds, np.int32))
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    return ctx.assoc_scores(aparams, points, off, N1, N2, desc)     # the host-pointer form: one block up, one call, one block back


def pairs_from_scores(score):
    """The augmented cost matrix — an option "no association" of cost 1 for every row and column — the Hungarian solve and the
    pair extraction [REF roman/map/global_nearest_neighbor.py:38-50] -> [(row, column), ...] in the reference's order."""
    from scipy.optimize import linear_sum_assignment
    score = np.asarray(score, dtype=np.float64)
    n1, n2 = score.shape
    cost = np.concatenate([np.concatenate([score, np.ones(score.shape)], axis=1), np.ones((n1, 2 * n2))], axis=0)
    rows, cols = linear_sum_assignment(cost)
    return [(int(r), int(c)) for r, c in zip(rows, cols) if r < n1 and c < n2]


def global_nearest_neighbor(clouds_a, clouds_b, params, ctx=None):
    """The reference's global_nearest_neighbor [REF roman/map/global_nearest_neighbor.py:5-50] over the device's score matrix ->
    the list of (index in clouds_a, index in clouds_b) that are associated."""
    return pairs_from_scores(association_scores(clouds_a, clouds_b, params, ctx=ctx).score)
