"""Submap-pair loop and result writers on the batched HIP path.

Mirrors the part of the reference's caller that surrounds the hot path:

  * `submap_align()` [REF roman/align/submap_align.py:74-220] in three forms that return the same `SubmapAlignResults` and leave
    the caller's submaps in the same state.  They share one skeleton: `_GridResults` holds the NaN-filled result matrices and
    builds the results object; pass 1 [REF :93-149] gates every pair of the S0 x S1 grid (distance / AABB, `skip_distance`,
    submap descriptor similarity: `_grid_similarity`, `_gates`) and `_GridResults.pass1()` is the one place where its outcome
    (`nearby`, `skip`, `gated`, the sentinels of [REF :179-184]) becomes matrix entries; the surviving pairs go to ONE batched
    device call over a pool that holds every submap once (`_drop_shared`, `_set_association_lists`, `_lc_inputs`); pass 2
    [REF :160-200] — gravity post-filters, error metrics against the reference transform — fills the rest.  The forms differ
    in where a step runs.  `submap_align()`, the pair loop, reads the submaps pair by pair in the reference's order, calls
    `roman_align_batch` and does pass 2 per pair on the host.  `submap_align_grid()` does pass 1 in NumPy over the whole grid
    and leaves pass 2 and the loop-closure edges to the device (`roman_align_lc_batch`, `_records_into_results`).
    `submap_align_pools()` starts from two device-resident submap pools (align.submaps.SubmapPool) and runs pass 1 on the
    device too (`roman_grid_gate_dev`), decoding its flags into the same `pass1()` call.
  * `save_submap_align_results()` [REF roman/align/results.py:122-194] — the `.g2o` loop-closure edges
    (`# LC: <n>` + `EDGE_SE3:QUAT`), the loop-closure json, the matrix pickle and the timing text, byte for byte
    in the reference's formats, and the per-robot `sm.json` dump ([REF :200-243]).  Plots and the pickled results
    object (which embeds reference classes) are left to the reference.

Loading ROMAN maps and ground-truth trajectories (robotdatapy, `roman.map`) is out of scope: the caller hands
over submap objects exposing the attributes of [REF roman/map/map.py:94-141] (`segments`, `pose_flu`,
`pose_flu_gt`, `descriptor`, `time`); `Submap` below is a minimal stand-in with the same semantics, including
the reference's quirk that `pose_gravity_aligned` flattens `pose_flu` IN PLACE [REF roman/utils.py:128-130].
"""
import copy
import json
import pickle
import time
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from .. import _abi
from ..runtime import LcInputs, LoopClosureResult, grid_gate_params, lc_record_dtype, stats_dtype
from .batch import AlignmentBatch, pack_submaps, run_batch, run_lc_batch, run_lc_batch_ids
from .dist_reg_with_pruning import DistRegWithPruning, _zyx_euler
from .object_registration import ObjectRegistration
from .ransac_reg import RansacReg


# ---------------------------------------------------------------------------------------------
# small SE(3) helpers (the reference takes them from robotdatapy.transform / roman.utils)
# ---------------------------------------------------------------------------------------------
def transform_rm_roll_pitch(T):
    """[REF roman/utils.py:128-130] — keeps yaw only; MUTATES and returns its argument, like the reference."""
    T[:3, :3] = Rot.from_euler('z', Rot.from_matrix(T[:3, :3]).as_euler('ZYX')[0]).as_matrix()
    return T


def transform_to_xyzrpy(T):
    """x, y, z, roll, pitch, yaw (fixed-axis xyz Euler angles, radians)."""
    return np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_euler('xyz')])


def transform_to_xyz_quat(T):
    """translation (3,), quaternion (4,) in xyzw order."""
    return T[:3, 3].copy(), Rot.from_matrix(T[:3, :3]).as_quat()


def aabb_intersects(p1, p2):
    """[REF roman/utils.py:160-169]"""
    p1_min, p1_max, p2_min, p2_max = np.min(p1, axis=0), np.max(p1, axis=0), np.min(p2, axis=0), np.max(p2, axis=0)
    return bool(np.all(p1_min[:3] <= p2_max[:3]) and np.all(p1_max[:3] >= p2_min[:3]))


def _zero_norm(norm_prod):
    """The reference's guard [REF roman/map/map.py:148-150, 159-160]: a cosine over such a product of norms is 0."""
    return np.isclose(norm_prod, 0.0, atol=1e-9, rtol=0.0)


@dataclass
class Submap:
    """Minimal stand-in for [REF roman/map/map.py:94-141]."""
    id: int
    time: float
    segments: List
    pose_flu: np.ndarray
    pose_flu_gt: Optional[np.ndarray] = None
    descriptor: Optional[np.ndarray] = None

    @property
    def pose_gravity_aligned(self):
        return transform_rm_roll_pitch(self.pose_flu)

    @property
    def pose_gravity_aligned_gt(self):
        return transform_rm_roll_pitch(self.pose_flu_gt)

    @property
    def position(self):
        return self.pose_flu[:3, 3]

    @property
    def position_gt(self):
        return self.pose_flu_gt[:3, 3]

    @property
    def has_gt(self):
        return self.pose_flu_gt is not None

    @property
    def segments_as_global_points(self):
        T = self.pose_gravity_aligned_gt if self.has_gt else self.pose_gravity_aligned
        pts = np.vstack([np.asarray(seg.center).reshape(1, -1)[:, :3] for seg in self.segments])
        return pts @ T[:3, :3].T + T[:3, 3]

    def __len__(self):
        return len(self.segments)

    @classmethod
    def similarity(cls, submap1, submap2):
        """[REF roman/map/map.py:144-162]: cosine, or maximum pairwise cosine for stacked descriptors."""
        desc1, desc2 = np.asarray(submap1.descriptor), np.asarray(submap2.descriptor)
        if desc1.ndim == desc2.ndim == 1:
            norm_prod = np.linalg.norm(desc1) * np.linalg.norm(desc2)
            if _zero_norm(norm_prod):
                return 0.0
            return np.dot(desc1, desc2) / norm_prod
        d1 = desc1.reshape(desc1.shape[0], 1, desc1.shape[1]); d2 = desc2.reshape(1, desc2.shape[0], desc2.shape[1])
        norm_prods = np.linalg.norm(d1, axis=2) * np.linalg.norm(d2, axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            sims = np.sum(d1 * d2, axis=2) / norm_prods
        sims[_zero_norm(norm_prods)] = 0.0
        return np.max(sims)


def _host_cosine(A, B):
    """What Context.cosine_matrix computes on the device, in NumPy (the CPU doubles' descriptor gate): (a, d) x (b, d) -> (a, b)."""
    norm_prod = np.linalg.norm(A, axis=1)[:, None] * np.linalg.norm(B, axis=1)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = (A @ B.T) / norm_prod
    sim[_zero_norm(norm_prod)] = 0.0
    return sim


def _grid_similarity(descs0, descs1, cosine):
    """Submap.similarity for every pair of the grid at once (row f2) -> (S0, S1), or None when the descriptors are of mixed kinds.
    `cosine(A, B)` is Context.cosine_matrix or _host_cosine: ONE call either way.  Vector descriptors: the cosine matrix itself.
    Stacked per-frame descriptors ([REF roman/map/map.py:152-162]: the best cosine over all frame pairs, zero-norm frames scoring
    0): all frames of all submaps at once, then a segmented maximum."""
    flat = descs0 + descs1
    if all(d.ndim == 1 for d in flat):
        return cosine(np.stack(descs0), np.stack(descs1))
    if all(d.ndim == 2 and d.shape[0] > 0 and d.shape[1] == flat[0].shape[1] for d in flat):
        o0 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs0])]).astype(np.int64)
        o1 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs1])]).astype(np.int64)
        frames = cosine(np.concatenate(descs0, axis=0), np.concatenate(descs1, axis=0))
        return np.maximum.reduceat(np.maximum.reduceat(frames, o0[:-1], axis=0), o1[:-1], axis=1)
    return None


def stacked_similarity(ctx, descs0, descs1):
    """Best pairwise cosine between the frame descriptors of every submap of robot 0 and every submap of robot 1
    ([REF roman/map/map.py:152-162]) -> (S0, S1).  One cosine kernel over all frames, then a segmented maximum."""
    return _grid_similarity(list(descs0), list(descs1), ctx.cosine_matrix)


def _device_cosine(registration):
    return lambda A, B: registration._context().cosine_matrix(A, B)      # (the context is made only if a cosine is asked for)


@dataclass
class SubmapAlignIO:
    """The fields of SubmapAlignInputOutput [REF roman/params/submap_align_params.py:153-198] the loop and the
    writers read."""
    robot_names: List[str] = field(default_factory=lambda: ["0", "1"])
    lc_association_thresh: int = 4
    g2o_t_std: float = 0.5
    g2o_r_std: float = float(np.deg2rad(0.5))
    skip_distance: float = np.inf
    gt_available: Sequence[bool] = (False, False)       # the reference tests `gt_pose_data[i] is not None`


@dataclass
class SubmapAlignResults:
    """Same fields as [REF roman/align/results.py:18-31]."""
    robots_nearby_mat: np.ndarray
    clipper_angle_mat: np.ndarray
    clipper_dist_mat: np.ndarray
    clipper_num_associations: np.ndarray
    similarity_mat: Optional[np.ndarray]
    submap_yaw_diff_mat: np.ndarray
    associated_objs_mat: list
    T_ij_mat: np.ndarray
    T_ij_hat_mat: np.ndarray
    timing_list: List[float]
    submap_align_params: object
    submap_io: object
    total_time: float = -np.inf
    # submap_align_grid / submap_align_pools only: the loop-closure edges as the device computed them — {'pairs': (K, 2) int (i, j) in loop order,
    # 't': (K, 3), 'q': (K, 4) xyzw}.  loop_closure_edges() and the writers then do no per-pair matrix work.
    lc_edges: Optional[dict] = None
    # submap_align_pools / submap_align_session with num_solutions=K only: {(i, j): [K tuples (associations, score, T_hat,
    # n_assoc, flags, edge)]} for every registered pair — every hypothesis of the pair, `edge` = (t (3,), q (4,) xyzw) of an ACCEPTED
    # hypothesis, else None.  The matrices above and lc_edges come from each pair's best hypothesis.
    hypotheses: Optional[dict] = None


# ---------------------------------------------------------------------------------------------
# what the three forms share: the result matrices, the rules of pass 1, the inputs of the batched call
# ---------------------------------------------------------------------------------------------
_NO_ESTIMATE = (180.0, 1e6)          # (theta, dist) of a pair without an estimate; it has 0 associations [REF :179-184]


def _edges_on_device(sm_io):
    return sm_io.lc_association_thresh > 0               # (a threshold <= 0 would accept pairs that never reach the device)


class _GridResults:
    """The result matrices of an (n0, n1) grid, NaN-filled as [REF roman/align/submap_align.py:80-91] allocates them; the rules
    that turn pass 1's outcome into their entries; the SubmapAlignResults at the end."""

    def __init__(self, sm_params, sm_io, n0, n1):
        nan = lambda *s: np.zeros(s) * np.nan
        self.sm_params, self.sm_io, self.t0 = sm_params, sm_io, time.time()
        self.clipper_angle_mat, self.clipper_dist_mat, self.clipper_num_associations = nan(n0, n1), nan(n0, n1), nan(n0, n1)
        self.similarity_mat, self.robots_nearby_mat, self.submap_yaw_diff_mat = nan(n0, n1), nan(n0, n1), nan(n0, n1)
        self.T_ij_mat, self.T_ij_hat_mat = nan(n0, n1, 4, 4), nan(n0, n1, 4, 4)
        self.associated_objs_mat = [[[] for _ in range(n1)] for _ in range(n0)]
        self.device_edges = _edges_on_device(sm_io)

    def empty_edges(self):
        return dict(pairs=np.zeros((0, 2), np.int64), t=np.zeros((0, 3)), q=np.zeros((0, 4))) if self.device_edges else None

    def pass1(self, dist, nearby, skip, gated, yaw_deg, sim, T_ij):
        """[REF :136-149, 179-184] over (n0, n1) arrays: `nearby` pairs get their distance and yaw difference; a pair beyond
        `skip_distance` (`skip`) has 0 associations and nothing else; every other pair gets its similarity, and one the
        descriptor gate stopped (`gated`) the sentinels of a pair without an estimate."""
        self.robots_nearby_mat[nearby] = dist[nearby]
        self.submap_yaw_diff_mat[nearby] = yaw_deg[nearby]
        self.T_ij_mat[:] = T_ij
        self.clipper_num_associations[skip] = 0
        self.similarity_mat[~skip] = sim[~skip]
        self.clipper_num_associations[gated] = 0
        self.clipper_angle_mat[gated & nearby] = np.abs(np.rad2deg(_NO_ESTIMATE[0])); self.clipper_dist_mat[gated & nearby] = _NO_ESTIMATE[1]

    def results(self, timing_list=(), lc_edges=None, hypotheses=None):
        return SubmapAlignResults(hypotheses=hypotheses,
            robots_nearby_mat=self.robots_nearby_mat, clipper_angle_mat=self.clipper_angle_mat, clipper_dist_mat=self.clipper_dist_mat,
            clipper_num_associations=self.clipper_num_associations,
            similarity_mat=self.similarity_mat if self.sm_params.submap_descriptor is not None else None,
            submap_yaw_diff_mat=self.submap_yaw_diff_mat, T_ij_mat=self.T_ij_mat, T_ij_hat_mat=self.T_ij_hat_mat,
            associated_objs_mat=self.associated_objs_mat, timing_list=list(timing_list), submap_align_params=self.sm_params,
            submap_io=self.sm_io, total_time=time.time() - self.t0, lc_edges=lc_edges)


def _gates(dist, sim, sm_params, sm_io):
    """The gate decisions of [REF :136-149] -> (skip, gated), for one pair or for arrays over the grid: beyond `skip_distance` a
    pair is skipped; otherwise the descriptor gate stops it below the threshold.  What neither holds for is registered."""
    skip = dist > sm_io.skip_distance
    with np.errstate(invalid="ignore"):
        gated = np.logical_not(skip) & (sim < sm_params.submap_descriptor_thresh)
    return skip, gated


def _drop_shared(segs_i, segs_j):
    """Self loop closures [REF :108-115]: both lists without the segments (by id) that both submaps hold."""
    common = {seg.id for seg in segs_i} & {seg.id for seg in segs_j}
    return [s for s in segs_i if s.id not in common], [s for s in segs_j if s.id not in common]


def _device_prefilter(registration):
    """A DistRegWithPruning whose prefilter the device evaluates (prune_on_device: ROMAN_INV_EUCLIDEAN_PRUNED):
    its `_associations_to_score` gives None for every pair.  A subclass that brings a scorer of its own is not one."""
    return (isinstance(registration, DistRegWithPruning) and bool(registration.prune_on_device)
            and type(registration)._associations_to_score is DistRegWithPruning._associations_to_score)


def _has_host_prefilter(registration):
    """A pruning plugin that scores explicit association lists: its host prefilter reads both maps of a pair.  Asked of the
    INSTANCE: a DistRegWithPruning with prune_on_device has none; any other plugin that overrides `_associations_to_score` has."""
    scorer = getattr(type(registration), "_associations_to_score", None)
    if scorer is None or scorer is ObjectRegistration._associations_to_score:
        return False
    return not _device_prefilter(registration)


def _set_association_lists(registration, batch, segs_of):
    """`batch.assoc` / `batch.assoc_off` from the registration's association list of every problem (`segs_of(b)` -> its two
    segment lists), all-to-all where it gives None for one; left unset when it gives None for all."""
    lists = [registration._association_list(*segs_of(b)) if (batch.n1[b] and batch.n2[b]) else None for b in range(len(batch))]
    if any(l is not None for l in lists):
        from ..clipperpy.utils import create_all_to_all
        lists = [l if l is not None else create_all_to_all(int(batch.n1[b]), int(batch.n2[b])) for b, l in enumerate(lists)]
        batch.assoc_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
        batch.assoc = np.concatenate(lists, axis=0).astype(np.int32)


def _tilt_thresh(registration):
    """DistRegWithPruning.register's own roll / pitch check [REF dist_reg_with_pruning.py:38-45], or None."""
    return registration.roll_pitch_thresh if getattr(registration, "use_gravity", False) else None


def _lc_inputs(sm_params, sm_io, registration, **arrays):
    """The switches of the device's loop-closure tail from the parameters; `arrays`: T_ref, enable, FL, iL, FR, iR where the host has them."""
    return LcInputs(dim=sm_params.dim, force_rm_upside_down=sm_params.force_rm_upside_down,
                    force_rm_lc_roll_pitch=sm_params.force_rm_lc_roll_pitch, tilt_thresh=_tilt_thresh(registration),
                    lc_association_thresh=int(np.ceil(sm_io.lc_association_thresh)) if _edges_on_device(sm_io) else 1, **arrays)


def submap_align(sm_params, submaps, sm_io: Optional[SubmapAlignIO] = None, registration=None,
                 compute: Optional[Callable] = None) -> SubmapAlignResults:
    """The pair loop of [REF roman/align/submap_align.py:74-220] over two lists of submaps, with ONE batched
    device call for all pairs that reach `register()`.

    `compute(registration, AlignmentBatch) -> runtime.BatchResult` defaults to the HIP path (`run_batch`); tests
    inject a CPU double.  `timing_list` gets the batch wall time divided evenly over the registered pairs (the
    reference times each `register()` call, [REF :155-157])."""
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    compute = compute or run_batch
    n0, n1 = len(submaps[0]), len(submaps[1])
    M = _GridResults(sm_params, sm_io, n0, n1)

    # ---- submap-descriptor gate (row f2): every cosine of the S0 x S1 gate in ONE device call (k_cos, f64 matrix core).
    # (The CPU test double, and descriptors of mixed kinds, use the per-pair definition below.) ----------------------
    sim_all = None
    if sm_params.submap_descriptor is not None and compute is run_batch and n0 and n1:
        sim_all = _grid_similarity(*[[np.asarray(sm.descriptor) for sm in submaps[r]] for r in range(2)], _device_cosine(registration))

    # ---- pass 1: gating, reference transforms, the list of pairs to register ([REF :93-149]), read pair by pair in the
    # reference's order (`pose_gravity_aligned[_gt]` flattens the pose it reads in place) ---------------------------------
    dist, yaw_deg, sim = np.full((n0, n1), np.nan), np.full((n0, n1), np.nan), np.full((n0, n1), np.inf)
    nearby, T_ij = np.zeros((n0, n1), dtype=bool), np.empty((n0, n1, 4, 4))
    for i in range(n0):
        for j in range(n1):
            si, sj = submaps[0][i], submaps[1][j]
            both_gt = si.has_gt and sj.has_gt
            dist[i, j] = np.linalg.norm(si.position_gt - sj.position_gt) if both_gt else np.linalg.norm(si.position - sj.position)
            nearby[i, j] = (not sm_params.force_fill_submaps and sm_params.submap_radius is not None and dist[i, j] < sm_params.submap_radius * 2) or \
                ((sm_params.force_fill_submaps or sm_params.submap_radius is None) and len(si) and len(sj)
                 and aabb_intersects(si.segments_as_global_points, sj.segments_as_global_points))
            T_wi = si.pose_gravity_aligned_gt if sm_io.gt_available[0] else si.pose_gravity_aligned
            T_wj = sj.pose_gravity_aligned_gt if sm_io.gt_available[1] else sj.pose_gravity_aligned
            T_ij[i, j] = np.linalg.inv(T_wi) @ T_wj
            if nearby[i, j]:
                yaw_deg[i, j] = np.abs(np.rad2deg(transform_to_xyzrpy(T_ij[i, j])[5]))
            if sm_params.submap_descriptor is not None:
                sim[i, j] = sim_all[i, j] if sim_all is not None else Submap.similarity(si, sj)
    skip, gated = _gates(dist, sim, sm_params, sm_io)
    M.pass1(dist, nearby, skip, gated, yaw_deg, sim, T_ij)
    todo = []                                            # (i, j, segs_i, segs_j), in loop order
    for i, j in np.argwhere(~skip & ~gated).tolist():
        segs_i, segs_j = list(submaps[0][i].segments), list(submaps[1][j].segments)
        todo.append((i, j) + (_drop_shared(segs_i, segs_j) if sm_params.single_robot_lc else (segs_i, segs_j)))

    # ---- the hot path: every submap (variant) packed once, one batched call ---------------------------------
    timing_list = []
    if todo:
        pool, index = [], {}

        def slot(key, segs):
            if key not in index:
                index[key] = len(pool); pool.append(segs)
            return index[key]
        shared = not sm_params.single_robot_lc           # without id removal a submap has ONE segment list
        ii = [slot((0, i) if shared else (0, i, j), si_) for (i, j, si_, _) in todo]
        jj = [slot((1, j) if shared else (1, i, j), sj_) for (i, j, _, sj_) in todo]
        feats, offs = pack_submaps(registration, pool)
        lens = np.diff(offs).astype(np.int32)
        batch = AlignmentBatch(feats, offs[ii].astype(np.int64), lens[ii], offs[jj].astype(np.int64), lens[jj])
        _set_association_lists(registration, batch, lambda b: todo[b][2:])
        t0 = time.time()
        res = compute(registration, batch)
        timing_list = [(time.time() - t0) / len(todo)] * len(todo)

    # ---- pass 2: post-filters, error metrics, result matrices ([REF :160-200]) ---------------------------------
    prune_tilt = _tilt_thresh(registration)
    for b, (i, j, _, _) in enumerate(todo):
        failed = bool(res.status[b] & (_abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_EMPTY_MAP))   # T_align would raise
        associations = res.assoc[b]
        if not failed:
            T_ij_hat = np.array(res.T[b], dtype=np.float64)
            if prune_tilt is not None:
                _, pitch, roll = _zyx_euler(T_ij_hat[:sm_params.dim, :sm_params.dim])
                failed = not (np.abs(roll) < prune_tilt and np.abs(pitch) < prune_tilt)
        if not failed:
            if sm_params.dim == 2:
                # The reference multiplies a 3x3 estimate into the 4x4 reference transform here and cannot run
                # ([REF :159-162]); the planar estimate is lifted to SE(3) (identity in z) instead.
                T2 = T_ij_hat; T_ij_hat = np.eye(4); T_ij_hat[:2, :2] = T2[:2, :2]; T_ij_hat[:2, 3] = T2[:2, 2]
                T_error = np.linalg.inv(T_ij_hat) @ T_ij[i, j]
                theta = np.arctan2(T_error[1, 0], T_error[0, 0]); d_err = np.linalg.norm(T_error[:2, 3])
            else:
                if sm_params.force_rm_upside_down:       # GravityConstraintError branch [REF :167-170]
                    xyzrpy = transform_to_xyzrpy(T_ij_hat)
                    failed = bool(np.abs(xyzrpy[3]) > np.deg2rad(90.) or np.abs(xyzrpy[4]) > np.deg2rad(90.))
                if not failed:
                    if sm_params.force_rm_lc_roll_pitch:
                        T_ij_hat = transform_rm_roll_pitch(T_ij_hat)
                    T_error = np.linalg.inv(T_ij_hat) @ T_ij[i, j]
                    theta = Rot.from_matrix(T_error[:3, :3]).magnitude(); d_err = np.linalg.norm(T_error[:3, 3])
        if failed:                                       # the except-branch sentinel [REF :179-184]
            T_ij_hat, (theta, d_err), associations = np.full((4, 4), np.nan), _NO_ESTIMATE, []
        if nearby[i, j]:
            M.clipper_angle_mat[i, j] = np.abs(np.rad2deg(theta)); M.clipper_dist_mat[i, j] = d_err
        M.clipper_num_associations[i, j] = len(associations)
        M.T_ij_hat_mat[i, j] = T_ij_hat
        M.associated_objs_mat[i][j] = associations
    return M.results(timing_list)


# ---------------------------------------------------------------------------------------------
# the grid form: pass 1 vectorised over the S0 x S1 grid, pass 2 and the edges behind the solver on the device
# ---------------------------------------------------------------------------------------------
def _read_times(sm, prop, attr, times):
    """Read `sm.<prop>` (`pose_gravity_aligned[_gt]`) `times` times, as the pair loop does — the stand-in Submap (like the
    reference's) rewrites `sm.<attr>` in place on every read.  Stops early once a read leaves the pose bitwise unchanged (a
    deterministic function applied to its own fixed point changes nothing), which a yaw-only pose does after one or two reads
    and a class that returns a copy does at once.  -> the last value read."""
    val = None
    for _ in range(int(times)):
        before = np.asarray(getattr(sm, attr)).tobytes()
        val = getattr(sm, prop)
        if np.asarray(getattr(sm, attr)).tobytes() == before:
            break
    return val


def _edge_frames(sm):
    """What loop_closure_edges() composes around the estimate for this submap — (inv(T_odom_p) @ T_odom_c,
    inv(T_odom_c) @ T_odom_p) — evaluated through the submap's OWN properties on a copy, so that a class whose
    `pose_gravity_aligned` flattens `pose_flu` in place (both then name the same matrix) gives what it gives there."""
    c = copy.copy(sm)
    c.pose_flu = np.array(sm.pose_flu, dtype=np.float64)
    T_c = c.pose_gravity_aligned
    T_p = c.pose_flu
    return np.linalg.inv(T_p) @ T_c, np.linalg.inv(T_c) @ T_p


def _quat_to_matrix(q):
    """(K, 4) xyzw unit quaternions -> (K, 3, 3)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _int64_ids(pool):
    """seg.id of every object of the pool, one per row, as int64 — or None when an id is not an integer int64 can hold (the
    device compares 64-bit integers; anything else keeps the set arithmetic of the host)."""
    out = []
    for segs in pool:
        for seg in segs:
            v = seg.id
            if not isinstance(v, (int, np.integer)) or not (-2 ** 63 <= int(v) < 2 ** 63):
                return None
            out.append(int(v))
    return np.array(out, dtype=np.int64)


def _records_into_results(M, res, ti, tj, nearby):
    """Pass 2 of the grid forms ([REF roman/align/submap_align.py:186-200]): the tail's records of the registered pairs (ti, tj)
    into the result matrices of `M`, IN PLACE -> the loop-closure edges (None unless the device decided them)."""
    rec = res.records
    if np.any(rec["flags"] & (_abi.ROMAN_LC_SKIPPED | _abi.ROMAN_LC_INTERNAL)):
        raise _abi.RomanHipError("the batched call left problems without a result (ROMAN_LC_SKIPPED / ROMAN_LC_INTERNAL records)")
    near = nearby[ti, tj]
    M.clipper_angle_mat[ti[near], tj[near]] = np.abs(np.rad2deg(rec["theta"][near]))
    M.clipper_dist_mat[ti[near], tj[near]] = rec["dist"][near]
    M.clipper_num_associations[ti, tj] = rec["n_assoc"]
    M.T_ij_hat_mat[ti, tj] = rec["T_hat"]
    failed = (rec["flags"] & _abi.ROMAN_LC_FAILED) != 0
    for b in np.nonzero(~failed)[0].tolist():            # (placing the association arrays: no arithmetic)
        M.associated_objs_mat[ti[b]][tj[b]] = res.assoc[b]
    if not M.device_edges:
        return None
    acc = np.asarray(res.accepted, dtype=np.int64)
    return dict(pairs=np.stack([ti[acc], tj[acc]], axis=1).astype(np.int64), t=np.array(rec["edge_t"][acc]), q=np.array(rec["edge_q"][acc]))


def submap_align_grid(sm_params, submaps, sm_io: Optional[SubmapAlignIO] = None, registration=None,
                      compute: Optional[Callable] = None) -> SubmapAlignResults:
    """submap_align() for callers that hand over the whole S0 x S1 grid: the same results (and the same state of the caller's
    submaps), with pass 1 ([REF roman/align/submap_align.py:93-149]) vectorised in NumPy over the grid and pass 2
    ([REF :160-200]) plus the loop-closure edges ([REF roman/align/results.py:156-171]) computed behind the solver on the device
    (roman_align_lc_batch).  Python loops run over SUBMAPS (packing, per-submap frames), never over pairs — except where a
    per-pair list is the input itself: a registration plugin's host prefilter.  The shared-segment removal of
    `single_robot_lc` ([REF :108-115]) runs on the device too (roman_align_lc_batch_ids: one id per pool row); it stays a
    per-pair host loop only with an injected `compute`, with such a plugin (its prefilter reads the reduced lists) or when
    an id is not an integer that int64 holds.  A DistRegWithPruning with prune_on_device has no host prefilter (the device applies
    it: `_has_host_prefilter` asks the instance) and takes the batched path, with no association lists.

    `compute(registration, AlignmentBatch, runtime.LcInputs) -> runtime.LoopClosureResult` defaults to the HIP path
    (`run_lc_batch`); tests inject a CPU double."""
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    if isinstance(registration, RansacReg):
        raise NotImplementedError("submap_align_grid builds on roman_align_lc_batch, which a RansacReg does not go through "
                                  "(use submap_align, or submap_align_pools over device-resident pools)")
    on_device = compute is None
    compute = compute or run_lc_batch
    S = [list(submaps[0]), list(submaps[1])]
    n0, n1 = len(S[0]), len(S[1])
    M = _GridResults(sm_params, sm_io, n0, n1)
    if n0 == 0 or n1 == 0:
        return M.results(lc_edges=M.empty_edges())

    # ---- per submap: sizes, positions, ground truth ---------------------------------------------------------
    lens = [np.array([len(sm) for sm in S[r]]) for r in range(2)]
    has_gt = [np.array([sm.has_gt for sm in S[r]], dtype=bool) for r in range(2)]
    pos = [np.stack([np.asarray(sm.position, dtype=np.float64) for sm in S[r]]) for r in range(2)]
    pos_gt = [np.stack([np.asarray(sm.position_gt, dtype=np.float64) if sm.has_gt else np.full(3, np.nan) for sm in S[r]]) for r in range(2)]
    both_gt = has_gt[0][:, None] & has_gt[1][None, :]
    with np.errstate(invalid="ignore"):
        dist = np.where(both_gt, np.linalg.norm(pos_gt[0][:, None, :] - pos_gt[1][None, :, :], axis=2),
                        np.linalg.norm(pos[0][:, None, :] - pos[1][None, :, :], axis=2))

    # ---- the in-place flattening of the pair loop, per submap: `pose_gravity_aligned[_gt]` rewrites the pose it reads, once
    # per pair the submap takes part in (and once more per AABB test); the count per pose is a function of the grid's shape ----
    aabb_mode = bool(sm_params.force_fill_submaps or sm_params.submap_radius is None)
    other = (n1, n0)
    boxes = [[None] * n0, [None] * n1]
    T_w = [[], []]
    for r in range(2):
        n_other_nonempty = int(np.count_nonzero(lens[1 - r]))
        for k, sm in enumerate(S[r]):
            n_aabb = n_other_nonempty if (aabb_mode and lens[r][k]) else 0
            uses = {"gt": 0, "flu": 0}
            uses["gt" if sm.has_gt else "flu"] += n_aabb
            uses["gt" if sm_io.gt_available[r] else "flu"] += other[r]
            if n_aabb:                                   # the global points of the first AABB test (one read of the pose)
                pts = sm.segments_as_global_points
                boxes[r][k] = (np.min(pts, axis=0)[:3], np.max(pts, axis=0)[:3])
                uses["gt" if sm.has_gt else "flu"] -= 1
            got = {}
            if uses["gt"]:
                got["gt"] = _read_times(sm, "pose_gravity_aligned_gt", "pose_flu_gt", uses["gt"])
            if uses["flu"]:
                got["flu"] = _read_times(sm, "pose_gravity_aligned", "pose_flu", uses["flu"])
            T_w[r].append(np.array(got["gt" if sm_io.gt_available[r] else "flu"], dtype=np.float64))
    T_w = [np.stack(T_w[r]) for r in range(2)]

    # ---- pass 1 over the grid: the radius / AABB gate, reference transforms, yaw differences, descriptor gate ----
    if not aabb_mode:
        nearby = dist < sm_params.submap_radius * 2
    else:
        nearby = np.zeros((n0, n1), dtype=bool)
        u0 = [k for k in range(n0) if boxes[0][k] is not None]; u1 = [k for k in range(n1) if boxes[1][k] is not None]
        if u0 and u1:
            lo0 = np.stack([boxes[0][k][0] for k in u0]); hi0 = np.stack([boxes[0][k][1] for k in u0])
            lo1 = np.stack([boxes[1][k][0] for k in u1]); hi1 = np.stack([boxes[1][k][1] for k in u1])
            hit = np.all(lo0[:, None, :] <= hi1[None, :, :], axis=2) & np.all(hi0[:, None, :] >= lo1[None, :, :], axis=2)
            nearby[np.ix_(u0, u1)] = hit
    T_ij = np.matmul(np.linalg.inv(T_w[0])[:, None, :, :], T_w[1][None, :, :, :])
    yaw = np.arctan2(T_ij[:, :, 1, 0], T_ij[:, :, 0, 0])              # the fixed-axis xyz yaw of a rotation about z
    if sm_params.submap_descriptor is None:
        sim = np.full((n0, n1), np.inf)
    else:                                                # row f2: every cosine of the gate in ONE call
        descs = [[np.asarray(sm.descriptor) for sm in S[r]] for r in range(2)]
        sim = _grid_similarity(descs[0], descs[1], _device_cosine(registration) if on_device else _host_cosine)
        if sim is None:                                  # mixed descriptor kinds: the per-pair definition
            sim = np.array([[Submap.similarity(si, sj) for sj in S[1]] for si in S[0]], dtype=np.float64)
    skip, gated = _gates(dist, sim, sm_params, sm_io)
    M.pass1(dist, nearby, skip, gated, np.abs(np.rad2deg(yaw)), sim, T_ij)
    ti, tj = np.nonzero(~skip & ~gated)                  # row-major: the order of the pair loop
    B = int(ti.shape[0])
    if B == 0:
        return M.results(lc_edges=M.empty_edges())

    # ---- the hot path: every submap (variant) packed once, ONE batched call with the tail behind it ---------
    host_lists = _has_host_prefilter(registration)
    ui, uj = np.unique(ti), np.unique(tj)
    pool = [list(S[0][i].segments) for i in ui] + [list(S[1][j].segments) for j in uj]
    pool_ids = None
    if sm_params.single_robot_lc and on_device and not host_lists:
        pool_ids = _int64_ids(pool)                      # self loop closures: the device drops the segments both submaps hold
    if not sm_params.single_robot_lc or pool_ids is not None:
        slot_i = np.zeros(n0, dtype=np.int64); slot_i[ui] = np.arange(len(ui))
        slot_j = np.zeros(n1, dtype=np.int64); slot_j[uj] = len(ui) + np.arange(len(uj))
        ii, jj = slot_i[ti], slot_j[tj]
    else:                                                # ... or the host does, per pair: a reduced copy of both submaps for every pair
        pool = [segs for i, j in zip(ti.tolist(), tj.tolist()) for segs in _drop_shared(list(S[0][i].segments), list(S[1][j].segments))]
        ii, jj = 2 * np.arange(B), 2 * np.arange(B) + 1
    feats, offs = pack_submaps(registration, pool)
    plen = np.diff(offs).astype(np.int32)
    batch = AlignmentBatch(feats, offs[ii].astype(np.int64), plen[ii], offs[jj].astype(np.int64), plen[jj],
                           pair_index=np.stack([ti, tj], axis=1), ids=pool_ids)
    if host_lists:
        _set_association_lists(registration, batch, lambda b: (pool[ii[b]], pool[jj[b]]))
    FL = np.tile(np.eye(4), (n0, 1, 1)); FR = np.tile(np.eye(4), (n1, 1, 1))
    for k in ui.tolist():
        FL[k] = _edge_frames(S[0][k])[0]
    for k in uj.tolist():
        FR[k] = _edge_frames(S[1][k])[1]
    times = [np.array([float(sm.time) for sm in S[r]]) for r in range(2)]
    enable = np.ones(B, dtype=np.int32)
    if sm_params.single_robot_lc:                        # the time gate of [REF roman/align/results.py:160-162]
        enable[np.abs(times[0][ti] - times[1][tj]) < sm_params.single_robot_lc_time_thresh] = 0
    lc = _lc_inputs(sm_params, sm_io, registration, T_ref=T_ij[ti, tj], enable=enable, FL=FL, iL=ti, FR=FR, iR=tj)
    t0 = time.time()
    res = run_lc_batch_ids(registration, batch, lc) if pool_ids is not None else compute(registration, batch, lc)
    timing_list = [(time.time() - t0) / B] * B

    # ---- pass 2: the records into the result matrices -------------------------------------------------------
    return M.results(timing_list, _records_into_results(M, res, ti, tj, nearby))


def _gate_buffers(torch, dev, n0, n1):
    """What roman_grid_gate_dev writes for an (n0, n1) grid, on `dev`, in the order of its output arguments: the dense matrices,
    and the compact list of the pairs to register with the tail's T_ref and enable (room for every pair)."""
    f64, i32, cap = torch.float64, torch.int32, n0 * n1
    spec = dict(dist=((n0, n1), f64), flags=((n0, n1), i32), yaw=((n0, n1), f64), sim=((n0, n1), f64), T_ij=((cap, 16), f64),
                pairs=((cap, 2), i32), T_ref=((cap, 16), f64), enable=((cap,), i32))
    g = {k: torch.empty(shape, dtype=t, device=dev) for k, (shape, t) in spec.items()}
    g["n_todo"] = torch.zeros(1, dtype=i32, device=dev)
    return g


class _TailBuffers:
    """The outputs of B problems over resident pools (issue_chunked) and of the tail behind them (roman_lc_tail_dev), on `dev`."""

    def __init__(self, torch, dev, B, kmax):
        f64, i32 = torch.float64, torch.int32
        self.assoc = torch.full((B, kmax, 2), -1, dtype=i32, device=dev); self.n = torch.zeros(B, dtype=i32, device=dev)
        self.T = torch.zeros((B, 16), dtype=f64, device=dev); self.status = torch.zeros(B, dtype=i32, device=dev)
        self.records = torch.zeros(B * _abi.LC_RECORD_NBYTES, dtype=torch.uint8, device=dev)
        self.acc_idx = torch.zeros(B, dtype=i32, device=dev); self.acc_n = torch.zeros(1, dtype=i32, device=dev)

    def result(self, status, dim, assoc=None):
        """-> runtime.LoopClosureResult on the host (`status`: the final status of every problem, as issue_chunked returns it;
        `assoc`: the association lists where the caller has read them back already, as the RANSAC path does chunk by chunk)."""
        B, s = int(self.n.shape[0]), dim + 1
        rec = np.frombuffer(self.records.cpu().numpy().tobytes(), dtype=lc_record_dtype()).copy()
        if assoc is None:
            n_h, a_h = self.n.cpu().numpy(), self.assoc.cpu().numpy()
            assoc = [a_h[b, :n_h[b]].copy() for b in range(B)]
        return LoopClosureResult(assoc, self.T.cpu().numpy()[:, :s * s].reshape(B, s, s).copy(), status,
                                 np.zeros(B, dtype=stats_dtype()), rec, self.acc_idx.cpu().numpy()[:int(self.acc_n.cpu().numpy()[0])].copy())


def reduced_problems(off1, n1, off2, n2, kept, region_row0):
    """The problem list behind roman_shared_reduce_dev (include/roman_hip.h), from the kept counts it wrote (`kept`: (B, 2)):
    a problem that lost an object on either side reads its fixed slots of the gather region — side 1 at row
    region_row0 + kb, side 2 n1 rows later, kb the sum of n1 + n2 over the problems in front — with n = kept (0: an empty map);
    every other problem is unchanged.  -> (off1, n1, off2, n2).  No loop over problems."""
    off1 = np.asarray(off1, dtype=np.int64); off2 = np.asarray(off2, dtype=np.int64)
    n1 = np.asarray(n1, dtype=np.int32); n2 = np.asarray(n2, dtype=np.int32)
    kept = np.asarray(kept, dtype=np.int32).reshape(-1, 2)
    if kept.shape[0] != n1.shape[0] or np.any(kept < 0) or np.any(kept[:, 0] > n1) or np.any(kept[:, 1] > n2):
        raise _abi.RomanHipError("roman_shared_reduce_dev: a kept count lies outside its map")
    tot = n1.astype(np.int64) + n2.astype(np.int64)
    kb = np.cumsum(tot) - tot
    lost = (kept[:, 0] != n1) | (kept[:, 1] != n2)
    return (np.where(lost, int(region_row0) + kb, off1), np.where(lost, kept[:, 0], n1).astype(np.int32),
            np.where(lost, int(region_row0) + kb + n1, off2), np.where(lost, kept[:, 1], n2).astype(np.int32))


# A RansacReg over resident pools: the association block of one roman_ransac_lc_batch_dev call (problems x kmax x 8 bytes, kmax the
# largest n1 * n2: every correspondence may be an inlier) stays under this many bytes; more problems go in several calls.
RANSAC_ASSOC_CHUNK_BYTES = 256 << 20


def _ransac_lc_over_pool(torch, ctx, registration, pool, batch, lp, o, tail_ptrs, wait_torch):
    """The RANSAC baseline for the problems of `batch` over the resident `pool` (rows of any width F >= 3 whose columns 0-2 are
    the centre: a pool built for any registration), DESIGN.md §4.13: roman_ransac_lc_batch_dev writes the split outputs into `o`
    (a _TailBuffers), the tail follows with `tail_ptrs` (T_ref, enable, frames).  One fused call when the association block of
    the whole batch fits RANSAC_ASSOC_CHUNK_BYTES; otherwise calls without a tail over chunks of problems — one chunk-sized
    association buffer, read back between them — and ONE roman_lc_tail_dev over all problems at the end.
    -> runtime.LoopClosureResult with ransac_records."""
    from ..runtime import ransac_kmax, ransac_record_dtype
    B, F, dev = len(batch), int(pool.shape[1]), pool.device
    rp = registration._ransac_params()
    kmax = ransac_kmax(batch.n1, batch.n2)
    chunk = max(1, int(RANSAC_ASSOC_CHUNK_BYTES // (8 * kmax)))
    nb = _abi.RANSAC_RECORD_NBYTES
    rec = torch.zeros(B * nb, dtype=torch.uint8, device=dev)
    rows = torch.full((min(B, chunk), kmax, 2), -1, dtype=torch.int32, device=dev)
    wait_torch()                                             # the cleared buffers are in place before the library's stream writes them
    assoc = []

    def harvest(lo, hi):                                     # after a sync: the chunk's counts, then only the columns that hold rows
        n = np.minimum(o.n[lo:hi].cpu().numpy(), kmax)
        a = rows[:hi - lo, :int(n.max())].cpu().numpy()
        assoc.extend(a[b, :n[b]].copy() for b in range(hi - lo))
    if chunk >= B:
        ctx.ransac_lc_batch_dev(rp, pool.data_ptr(), F, batch.off1, batch.n1, batch.off2, batch.n2, kmax, rows.data_ptr(), rec.data_ptr(),
                                T_out_ptr=o.T.data_ptr(), n_assoc_out_ptr=o.n.data_ptr(), status_out_ptr=o.status.data_ptr(), lc_params=lp,
                                records_ptr=o.records.data_ptr(), accepted_idx_ptr=o.acc_idx.data_ptr(), n_accepted_ptr=o.acc_n.data_ptr(), **tail_ptrs)
        ctx.sync()
        harvest(0, B)
    else:
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            ctx.ransac_lc_batch_dev(rp, pool.data_ptr(), F, batch.off1[lo:hi], batch.n1[lo:hi], batch.off2[lo:hi], batch.n2[lo:hi], kmax,
                                    rows.data_ptr(), rec.data_ptr() + lo * nb, T_out_ptr=o.T.data_ptr() + lo * 128,
                                    n_assoc_out_ptr=o.n.data_ptr() + lo * 4, status_out_ptr=o.status.data_ptr() + lo * 4)
            ctx.sync()
            harvest(lo, hi)
        ctx.lc_tail_dev(lp, B, o.T.data_ptr(), o.n.data_ptr(), o.status.data_ptr(), o.records.data_ptr(), o.acc_idx.data_ptr(), o.acc_n.data_ptr(),
                        **tail_ptrs)
        ctx.sync()
    res = o.result(o.status.cpu().numpy().copy(), 3, assoc=assoc)
    res.ransac_records = np.frombuffer(rec.cpu().numpy().tobytes(), dtype=ransac_record_dtype()).copy()
    return res


def _pool_side_host(pool, gt_poses, gt_available, reads, aabb_mode):
    """The O(S) host block of one side of submap_align_pools / one robot of submap_align_session, over the non-empty submaps of
    `pool`: centre, the pose the reference transform is built from, time, the edge frames — through the stand-in Submap's own
    properties, read as often as the pair loop reads them (submap_align_grid does the same).  `reads`: ascending numbers of
    submaps on the other side; T_w and the edge frames are given after each of them (a deterministic function applied n times: reading on
    from one entry to the next gives what n reads from the start give).  -> dict(pos (S, 3), pos_gt (S, 3) or None, time (S,),
    T_oc (S, 4, 4) or None, and per entry of reads: T_w [(S, 4, 4)], frames [((S, 4, 4) left, (S, 4, 4) right)])."""
    c = pool.centers
    gt = None if gt_poses is None else np.asarray(gt_poses, dtype=np.float64).reshape(len(c), 4, 4)
    sms = [Submap(id=int(s), time=float(c.time[s]), segments=(), pose_flu=np.array(c.pose_flu[s], dtype=np.float64),
                  pose_flu_gt=None if gt is None else gt[s].copy()) for s in pool.nonempty]
    pos = np.stack([np.array(sm.position) for sm in sms])
    pos_gt = None if gt is None else np.stack([np.array(sm.position_gt) for sm in sms])
    # the AABB gate reads the pose once more per submap, in front of the pair loop (segments_as_global_points, by has_gt
    # [REF roman/map/map.py:138]).  The pools' poses are yaw-only COPIES already, so how often the pair loop flattens them in
    # place does not matter here: _read_times below stops at the fixed point either way
    T_oc = None if not aabb_mode else np.stack([np.array(sm.pose_gravity_aligned_gt if sm.has_gt else sm.pose_gravity_aligned, dtype=np.float64) for sm in sms])
    read = ("pose_gravity_aligned_gt", "pose_flu_gt") if gt_available else ("pose_gravity_aligned", "pose_flu")
    T_w, frames, done = [], [], 0
    for n in reads:                                          # (cumulative: the reads of one entry continue those of the entry before)
        if n > done:
            vals = [_read_times(sm, *read, n - done) for sm in sms]
            T_w.append(np.stack([np.array(v, dtype=np.float64) for v in vals]))
            fr = [_edge_frames(sm) for sm in sms]            # (on a copy of the submap as the reads left it)
            frames.append((np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])))
        else:
            T_w.append(T_w[-1]); frames.append(frames[-1])
        done = n
    times = np.array([sm.time for sm in sms], dtype=np.float64)
    return dict(pos=pos, pos_gt=pos_gt, T_w=T_w, time=times, T_oc=T_oc, frames=frames)


# ---------------------------------------------------------------------------------------------
# the stages submap_align_pools and submap_align_session share: refusals, device plumbing, the read-back of pass 1, the
# shared-segment removal and the registration over resident rows.  submap_align_session and submap_align_session_update share
# every stage of a session call but the gate and its read-back, further down: _session_setup (arguments and early refusals),
# _session_views, _session_block_results, _session_context (the refusals that ask the context), _session_uploads, _session_pool,
# _session_pass1_front (boxes and stacked similarity in front of the gate) and _session_register (all blocks in one batch)
# ---------------------------------------------------------------------------------------------
def _no_device(registration, p):
    """No context of the caller's and host-tensor pools: nothing a kernel could run on."""
    return getattr(registration, "_ctx", None) is None and any(q.pool.device.type == "cpu" for q in p)


def _ransac_refusals(registration, p, way):
    """What a RansacReg over the pools `p` is refused for — every check in front of registration._context() makes no HIP context."""
    if any(int(q.table.point_dim) != 3 for q in p):
        raise ValueError("RansacReg reads x y z from columns 0-2 of a pool row, and pools of dim 2 hold no z" + way)
    if any(int(q.cap) > _abi.ROMAN_RANSAC_MAX_OBJECTS for q in p):
        raise ValueError(f"RansacReg serves at most {_abi.ROMAN_RANSAC_MAX_OBJECTS} objects per submap (the pools' cap is larger)" + way)
    if _no_device(registration, p):
        raise ValueError("RansacReg has no context set and the pools are host tensors: no device to run on" + way)
    if not hasattr(registration._context(), "ransac_lc_batch_dev"):
        raise ValueError("the context has no roman_ransac_lc_batch_dev" + way)


def _mno_refusals(registration, p, pool_pairs, num_solutions, way):
    """What num_solutions=K over the pools `p` is refused for (`pool_pairs`: the (r, s) to align) — in front of anything that makes a HIP
    context: a RansacReg builds no affinity matrix to take a second solution from; K outside 1 ... ROMAN_MNO_MAX_SOLUTIONS; a `cap`
    whose all-to-all list exceeds what roman_mno_batch serves per problem."""
    if isinstance(registration, RansacReg):
        raise ValueError("num_solutions needs a CLIPPER method: RansacReg builds no affinity matrix" + way)
    K = num_solutions
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not (1 <= int(K) <= _abi.ROMAN_MNO_MAX_SOLUTIONS):
        raise ValueError(f"num_solutions must be an integer in 1 ... {_abi.ROMAN_MNO_MAX_SOLUTIONS} (got {K!r})" + way)
    for r, s_ in pool_pairs:
        if int(p[r].cap) * int(p[s_].cap) > _abi.ROMAN_MNO_MAX_ASSOC:
            raise ValueError(f"num_solutions: submaps of up to {int(p[r].cap)} x {int(p[s_].cap)} objects have an all-to-all list above the "
                             f"{_abi.ROMAN_MNO_MAX_ASSOC} associations roman_mno_batch serves per problem (ROMAN_MNO_MAX_ASSOC)" + way)


def _prune_refusals(registration, p, way):
    """What a device-prefilter plugin (DistRegWithPruning.on_device()) over the pools `p` is refused for, in front of anything that
    makes a HIP context: the cosine stage reads [centre | volume, linearity, planarity, scattering | descriptor] from every row, and
    rows packed by another registration (another number of shape columns, or method='roman': the same number in another order)
    would be read as they lie — shape attributes out of descriptor columns, a volume for a linearity — without any error."""
    d = registration.semantics_dim
    if d is None:
        raise ValueError("the device prefilter needs the descriptor length: DistRegWithPruning.on_device(semantics_dim=...) before the pools are built" + way)
    F = int(registration.dim) + 4 + int(d)
    if any(int(q.pool.shape[1]) != F for q in p):
        raise ValueError(f"the device prefilter reads rows of dim + 4 + semantics_dim = {F} columns [centre | volume, linearity, planarity, scattering | "
                         "descriptor]: build the pools with MapTable.from_segments(registration.on_device(semantics_dim), segments)" + way)
    if any(int(q.table.desc_dim) != int(d) for q in p):
        raise ValueError(f"the device prefilter contracts descriptors of semantics_dim = {int(d)}, and a pool's table was packed with another desc_dim" + way)
    # (method='roman' packs [centre | linearity, planarity, scattering | volume | descriptor]: the same width, another column order)
    if any(getattr(q.table, "invariant", None) not in (None, _abi.ROMAN_INV_EUCLIDEAN_PRUNED) for q in p):
        raise ValueError("a pool's table was packed by another registration, with its own column order between centre and descriptor: build the "
                         "pools with MapTable.from_segments(registration.on_device(semantics_dim), segments)" + way)


def _descriptor_refusals(registration, p, mode, way):
    """The descriptor modes the pools `p` do not carry, and a plugin whose host prefilter would need the segment rows back."""
    if mode not in (None, 'mean_semantic', 'mean_frame_descriptor', 'stacked_frame_descriptors'):
        raise ValueError(f"submap_descriptor {mode!r} is not one the pools carry" + way)
    if mode in ('mean_frame_descriptor', 'stacked_frame_descriptors') and any(q.descriptor_mode != mode for q in p):
        raise ValueError(f"submap_descriptor {mode!r} needs pools built with it (build_submap_pool(frames=...) keeps the frame masks on the device)" + way)
    if _has_host_prefilter(registration):
        raise ValueError("the registration plugin prefilters association lists on the host" + way)


def _descriptor_dim(p, mode, the_pools, way):
    """-> the length of the submap descriptors the gate contracts: 0 without a descriptor, and for stacked frame descriptors (the
    gate then reads a ready similarity).  Refuses pools `p` (`the_pools` in the text) that lack them or disagree on the length."""
    if mode is None or not p:
        return 0
    if mode == 'stacked_frame_descriptors':
        if any(int(q.frame_desc_dev.shape[1]) != int(p[0].frame_desc_dev.shape[1]) for q in p):
            raise ValueError(f"{the_pools} have frame descriptors of different lengths" + way)
        return 0
    if any(q.desc_dev is None for q in p):
        raise ValueError(f"submap_descriptor {mode!r} needs pools built with it (build_submap_pool keeps the descriptors on the device)" + way)
    d = int(p[0].desc_dev.shape[1])
    if any(int(q.desc_dev.shape[1]) != d for q in p):
        raise ValueError(f"{the_pools} have descriptors of different lengths" + way)
    return d


def _plumbing(torch, dev):
    """-> (wait_torch, up, ptr) for pools on `dev` (CPU tensors: a stand-in context, as the tests use): wait_torch() returns when
    torch's stream has done what was asked of it — the library's stream may read it then —, up(array or None) -> tensor on `dev`,
    ptr(tensor or None) -> address."""
    wait_torch = (lambda: None) if dev.type == "cpu" else (lambda: torch.cuda.current_stream(dev).synchronize())
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    return wait_torch, up, ptr


def _pass1_block(M, h, lo, hi, n0, n1, compact_pairs, what):
    """Pass 1 of one (n0, n1) grid as the gate left it at [lo, hi) of its dense outputs `h` (host arrays), into `M`.  `compact_pairs`:
    the grid's rows of the compact list, grid-local; they must be the TODO pairs in row-major order (`what`: the text of the
    error otherwise).  -> (nearby, todo), (n0, n1) bool."""
    cut = lambda k: h[k].reshape(-1)[lo:hi].reshape(n0, n1)
    flags = cut("flags")
    nearby, todo = (flags & _abi.ROMAN_GRID_NEARBY) != 0, (flags & _abi.ROMAN_GRID_TODO) != 0
    M.pass1(cut("dist"), nearby, (flags & _abi.ROMAN_GRID_SKIP) != 0, (flags & _abi.ROMAN_GRID_GATED) != 0, cut("yaw"), cut("sim"),
            h["T_ij"][lo:hi].reshape(n0, n1, 4, 4))
    if not np.array_equal(compact_pairs, np.stack(np.nonzero(todo), axis=1)):
        raise _abi.RomanHipError(what)
    return nearby, todo


def _drop_shared_over_pool(torch, ctx, pool, ids_dev, off1, n1, off2, n2, sel, wait_torch):
    """The shared-segment removal of [REF roman/align/submap_align.py:108-115] for the problems `sel` of (off1, n1, off2, n2) over
    the resident rows `pool` (`ids_dev`: one id per row), DESIGN.md §4.11: the pool's rows and behind them the fixed slots of
    THESE problems' gather region in ONE allocation; mark + gather in one launch; the kept counts back (8 bytes per problem: the
    one extra synchronisation).  The problems that lost something then read their slots, the others the pool as given.
    -> (pool with the region, off1, n1, off2, n2)."""
    rows, F, dev = int(pool.shape[0]), int(pool.shape[1]), pool.device
    sub = [np.ascontiguousarray(a[sel]) for a in (off1, n1, off2, n2)]
    n_slots = int(sub[1].sum(dtype=np.int64) + sub[3].sum(dtype=np.int64))
    work = torch.empty((rows + n_slots, F), dtype=torch.float64, device=dev)
    work[:rows].copy_(pool)
    keep_dev = torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev); kept_dev = torch.zeros((len(sel), 2), dtype=torch.int32, device=dev)
    wait_torch()                                             # the copy of the pool and the ids are in place
    ctx.shared_reduce_dev(len(sel), F, work.data_ptr(), rows, ids_dev.data_ptr(), *sub, keep_dev.data_ptr(), kept_dev.data_ptr())
    ctx.sync()
    out = [np.array(a) for a in (off1, n1, off2, n2)]
    for a, red in zip(out, reduced_problems(*sub, kept_dev.cpu().numpy(), rows)):
        a[sel] = red
    return (work, *out)


def _mno_lc_over_pool(torch, ctx, registration, pool, batch, K, kmax, lp, B, tail_ptrs, dim):
    """num_solutions=K: the K solves of every problem over the resident rows (pipeline.issue_mno_chunked: chunks,
    skipped problems issued again), join, ONE roman_mno_lc_tail_dev over the final block.  -> runtime.LoopClosureResult whose
    entry b is problem b's BEST hypothesis (hypothesis 0's record — a failed one, the sentinels — where best = -1) and whose
    accepted list is accepted_best_idx, with `.hypotheses`: per problem the K tuples of SubmapAlignResults.hypotheses."""
    from .pipeline import issue_mno_chunked
    from ..runtime import mno_solution_dtype
    dev, i32 = pool.device, torch.int32
    a_out = torch.full((B, K, kmax, 2), -1, dtype=i32, device=dev)
    sol = torch.zeros(B * K * _abi.MNO_SOLUTION_NBYTES, dtype=torch.uint8, device=dev)
    rec = torch.zeros(B * K * _abi.LC_RECORD_NBYTES, dtype=torch.uint8, device=dev)
    best = torch.full((B,), -1, dtype=i32, device=dev)
    idx = torch.zeros(B * K, dtype=i32, device=dev); cnt = torch.zeros(1, dtype=i32, device=dev)
    bidx = torch.zeros(B, dtype=i32, device=dev); bcnt = torch.zeros(1, dtype=i32, device=dev)
    status = issue_mno_chunked(ctx, registration._abi_params(), pool, batch, K, kmax, a_out, sol)   # re-issues skipped problems, then synchronises:
    ctx.join()                                               # ... the tail below sees the FINAL attempt of every problem only
    ctx.mno_lc_tail_dev(lp, B, K, sol.data_ptr(), rec.data_ptr(), best.data_ptr(), idx.data_ptr(), cnt.data_ptr(), bidx.data_ptr(), bcnt.data_ptr(),
                        **tail_ptrs)
    ctx.sync()
    s = dim + 1
    sol_h = np.frombuffer(sol.cpu().numpy().tobytes(), dtype=mno_solution_dtype()).reshape(B, K)
    rec_h = np.frombuffer(rec.cpu().numpy().tobytes(), dtype=lc_record_dtype()).reshape(B, K).copy()
    best_h, a_h = best.cpu().numpy(), a_out.cpu().numpy()
    if np.any(rec_h["flags"] & (_abi.ROMAN_LC_SKIPPED | _abi.ROMAN_LC_INTERNAL)):       # (on ANY hypothesis: the best view below would hide one behind k = 0)
        raise _abi.RomanHipError("the multi-solution call left hypotheses without a result (ROMAN_LC_SKIPPED / ROMAN_LC_INTERNAL records)")
    rows = np.minimum(sol_h["n_assoc"], kmax)
    hyps = []
    for b in range(B):
        one = []
        for k in range(K):
            r = rec_h[b, k]
            edge = (r["edge_t"].copy(), r["edge_q"].copy()) if r["flags"] & _abi.ROMAN_LC_ACCEPTED else None
            one.append((a_h[b, k, :rows[b, k]].copy(), float(sol_h["score"][b, k]), r["T_hat"].copy(), int(r["n_assoc"]), int(r["flags"]), edge))
        hyps.append(one)
    pick = np.maximum(best_h, 0)
    ar = np.arange(B)
    res = LoopClosureResult([hyps[b][pick[b]][0] for b in range(B)], sol_h["T"][ar, pick][:, :s * s].reshape(B, s, s).copy(), status,
                            np.zeros(B, dtype=stats_dtype()), rec_h[ar, pick].copy(), bidx.cpu().numpy()[:int(bcnt.cpu().numpy()[0])].copy())
    res.hypotheses, res.best = hyps, best_h
    return res


def _hypotheses_of(res, ti, tj):
    """SubmapAlignResults.hypotheses of the registered pairs (ti, tj), or None on the single-solution path."""
    hyps = getattr(res, "hypotheses", None)
    return None if hyps is None else {(int(i), int(j)): h for i, j, h in zip(ti, tj, hyps)}


def _register_over_pool(torch, ctx, registration, sm_params, sm_io, pool, batch, kmax, g, B, FL, FR, wait_torch, num_solutions=None):
    """The B problems of `batch` over the resident rows `pool`, and the tail behind them with T_ref, enable and the pairs where the
    gate wrote them (`g`) and the edge frames FL / FR (device tensors, indexed by the pairs): issue_chunked, join and
    roman_lc_tail_dev — or, for a RansacReg, `_ransac_lc_over_pool`.  -> (runtime.LoopClosureResult, seconds per pair)."""
    from .pipeline import issue_chunked
    ransac = isinstance(registration, RansacReg)
    o = _TailBuffers(torch, pool.device, B, 0 if ransac else kmax)   # (a RansacReg keeps its association rows in a buffer of its own)
    iL, iR = g["pairs"][:B, 0].contiguous(), g["pairs"][:B, 1].contiguous()
    lp = _lc_inputs(sm_params, sm_io, registration).params()
    tail_ptrs = dict(T_ref_ptr=g["T_ref"].data_ptr(), enable_ptr=g["enable"].data_ptr(), FL_ptr=FL.data_ptr(), iL_ptr=iL.data_ptr(),
                     FR_ptr=FR.data_ptr(), iR_ptr=iR.data_ptr())
    wait_torch()                                             # the pool (torch.cat), the cleared outputs and the frames are in place
    t0 = time.time()
    if ransac:                                               # k_ransac over the rows as they are, the tail behind it
        res = _ransac_lc_over_pool(torch, ctx, registration, pool, batch, lp, o, tail_ptrs, wait_torch)
    elif num_solutions is not None:                          # K hypotheses per pair, the tail over all of them, the best of each pair
        res = _mno_lc_over_pool(torch, ctx, registration, pool, batch, int(num_solutions), kmax, lp, B, tail_ptrs, sm_params.dim)
    else:
        status = issue_chunked(ctx, registration._abi_params(), pool, batch, kmax, o.assoc, o.n, o.T, o.status)   # re-issues skipped problems, then synchronises:
        ctx.join()                                           # ... the tail below sees the FINAL attempt of every problem only
        ctx.lc_tail_dev(lp, B, o.T.data_ptr(), o.n.data_ptr(), o.status.data_ptr(), o.records.data_ptr(), o.acc_idx.data_ptr(), o.acc_n.data_ptr(), **tail_ptrs)
        ctx.sync()
        res = o.result(status, sm_params.dim)
    return res, (time.time() - t0) / B


def submap_align_pools(sm_params, pools, sm_io: Optional[SubmapAlignIO] = None, registration=None, gt_poses=(None, None),
                       num_solutions=None) -> SubmapAlignResults:
    """submap_align_grid() for two maps whose submaps are ALREADY in HBM (`pools`: two align.submaps.SubmapPool, as
    build_submap_pool leaves them): the same results as submap_align_grid(sm_params, [p.to_submaps(segments) for p in pools]),
    without a segment row coming back to the host or going up twice.  Pass 1 ([REF roman/align/submap_align.py:93-149])
    is ONE device call over the grid of the non-empty submaps (roman_grid_gate_dev: radius gate, reference transforms, yaw
    differences, descriptor gate, the pairs to register in loop order with the tail's T_ref and enable); the host uploads the
    per-submap arrays (centres, poses, times: O(S)) and reads back the pair list and the S0 x S1 matrices.  The pairs then run
    over the resident pools (pipeline.issue_chunked), the tail over the final outputs (roman_ctx_join, roman_lc_tail_dev) with
    T_ref and enable where the gate wrote them.

    gt_poses[r]: None, or (S, 4, 4) ground-truth `pose_flu_gt` of EVERY centre of pool r (empty submaps included) — then every
    submap of that side has ground truth ([REF :96-99]); sm_io.gt_available[r] selects it for the reference transform.

    Self loop closures (`single_robot_lc` over pools that share segment ids — one pool against itself: submap_align_pools(p,
    [pool, pool])): the shared-segment removal of [REF :108-115] runs over the resident pools (roman_shared_reduce_dev, DESIGN.md
    §4.11: the ids build_submap_pool kept on the device, one launch, 8 bytes per pair back); returned associations index the
    reduced lists, as the reference's do.  Pools that share no id take the path without it.

    force_fill_submaps / no submap_radius: the gate is aabb_intersects over segments_as_global_points
    [REF :101-103].  Per side the host resolves T_odom_center (the ground-truth pose where gt_poses[r] is given, as `has_gt` does
    [REF roman/map/map.py:138]); roman_submap_boxes_dev reduces every submap of either pool to its box, roman_grid_gate_aabb_dev
    is the gate — behind roman_stacked_sim_dev for stacked descriptors — all on the context's stream.  Pools built by
    build_submap_pool(fill=...) (force-fill slices) and radius-mode pools are served alike.

    Not covered — ValueError; SubmapPool.to_submaps() + submap_align_grid is the way: the AABB gate over pools with dim 2 (their
    rows hold no z) or a context without roman_grid_gate_aabb_dev, registration plugins whose prefilter runs on the host (their pool
    rows hold centres only; for method='clipper+prune' DistRegWithPruning.on_device() gives the plugin that is served, below),
    shared ids over pools without `ids_dev`.

    method='clipper+prune'  runs with the device-prefilter plugin, `reg = sm_params.get_object_registration()
    .on_device(semantics_dim)`, over pools built with it (MapTable.from_segments(reg, segments): rows [centre | volume, linearity,
    planarity, scattering | descriptor]), in every mode above: both gates, every submap descriptor, [pool, pool] self loop closures
    (the gather region holds the full-width rows).  It is a CLIPPER method like any other here — issue_chunked with
    ROMAN_INV_EUCLIDEAN_PRUNED, join, the tail with the plugin's roll / pitch check.  Refused for it, before a context is made
    (`_prune_refusals`, four): semantics_dim unset, pools of another row width than dim + 4 + semantics_dim, a table of another
    desc_dim, a table packed by another registration (MapTable.invariant: method='roman' rows have the same width and another
    column order).  The factory's own plugin (prune_on_device=False) keeps its NumPy prefilter and stays refused.

    A RansacReg (method='ransac') runs over the same pools — built with ANY registration: roman_ransac_lc_batch_dev
    reads the centre from columns 0-2 of a row and nothing else — with pass 1 and the shared-segment removal unchanged; in place
    of issue_chunked, join and the tail there are RANSAC calls (chunked by RANSAC_ASSOC_CHUNK_BYTES) and one tail
    (`_ransac_lc_over_pool`).  Refused for it: pools of dim 2, a `cap` above ROMAN_RANSAC_MAX_OBJECTS, a context without
    roman_ransac_lc_batch_dev, and host-tensor pools while the registration has no context set.

    Frame descriptors need pools built with them (build_submap_pool(frames=...)): 'mean_frame_descriptor' goes
    through the same gate as 'mean_semantic'; 'stacked_frame_descriptors' through roman_stacked_sim_dev over the two pools' frame
    masks — every distinct frame pair contracted once — and roman_grid_gate_sim_dev on that similarity.  similarity_mat is what
    the device computed.

    num_solutions=K (1 ... 64): every registered pair gets K hypotheses (roman_mno_batch_dev over the resident rows
    in chunks, skipped problems issued again) and ONE roman_mno_lc_tail_dev runs the tail over all of them.  The result matrices
    and lc_edges come from each pair's best hypothesis — no failed filter, most associations, the lower k among equals; the
    reference's sentinels where every hypothesis failed — and `hypotheses` holds all K per pair.  Every hypothesis is a plain-CLIPPER
    solve over all associations: for a method with single scores (`roman`) hypothesis 0 is in general not register()'s result.
    Refused before a context is made: a RansacReg, K outside 1 ... 64, a pool `cap` whose all-to-all list exceeds
    ROMAN_MNO_MAX_ASSOC; after it: a context without roman_mno_lc_tail_dev.  None: the single-solution path, unchanged."""
    import torch
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    way = " (not on the device-resident path: use SubmapPool.to_submaps() + submap_align_grid)"
    p = list(pools)
    if len(p) != 2:
        raise ValueError("pools must hold two SubmapPool objects")
    if num_solutions is not None:
        _mno_refusals(registration, p, [(0, 1)], num_solutions, way)
    if isinstance(registration, RansacReg):
        _ransac_refusals(registration, p, way)
    if _device_prefilter(registration):
        _prune_refusals(registration, p, way)
    aabb_mode = bool(sm_params.force_fill_submaps or sm_params.submap_radius is None)
    mode = sm_params.submap_descriptor
    stacked = mode == 'stacked_frame_descriptors'
    _descriptor_refusals(registration, p, mode, way)
    d = _descriptor_dim(p, mode, "the two pools", "")
    for r in range(2):
        if sm_io.gt_available[r] and gt_poses[r] is None:
            raise ValueError(f"sm_io.gt_available[{r}] is set without gt_poses[{r}]")
    ctx = registration._context()
    if num_solutions is not None and not hasattr(ctx, "mno_lc_tail_dev"):
        raise ValueError("the context has no roman_mno_lc_tail_dev" + way)
    if aabb_mode and not (hasattr(ctx, "grid_gate_aabb_dev") and hasattr(ctx, "submap_boxes_dev")):
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes" + way)
    if aabb_mode and any(int(q.table.point_dim) != 3 for q in p):
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes, and pools of dim 2 hold no z" + way)
    # self loop closures over submaps that share segment ids: the removal of [REF :108-115] runs over the resident pools too
    # (roman_shared_reduce_dev) — with the ids build_submap_pool left on the device
    shared = bool(sm_params.single_robot_lc) and (p[0] is p[1] or np.intersect1d(p[0].ids[p[0].src >= 0], p[1].ids[p[1].src >= 0]).size > 0)
    if shared and (any(q.ids_dev is None for q in p) or not hasattr(ctx, "shared_reduce_dev")):
        raise ValueError("single_robot_lc over submaps that share segment ids needs pools that kept their ids on the device (SubmapPool.ids_dev, "
                         "as build_submap_pool leaves it) and a context with roman_shared_reduce_dev" + way)
    dev = p[0].pool.device
    wait_torch, up, ptr = _plumbing(torch, dev)
    keep = [q.nonempty for q in p]                           # [REF roman/map/map.py:341]: the reference drops the empty submaps
    n0, n1 = len(keep[0]), len(keep[1])
    M = _GridResults(sm_params, sm_io, n0, n1)
    if n0 == 0 or n1 == 0:
        return M.results(lc_edges=M.empty_edges(), hypotheses=None if num_solutions is None else {})

    # ---- per submap, on the host (O(S)): centre, the pose the reference transform is built from, time, the edge frames —
    # through the stand-in Submap's own properties, read as often as the pair loop reads them (submap_align_grid does the same) ----
    other = (n1, n0)
    side, frames = [], []
    for r in range(2):
        hs = _pool_side_host(p[r], gt_poses[r], sm_io.gt_available[r], [other[r]], aabb_mode)
        frames.append(hs["frames"][0][r])
        side.append(dict(pos=up(hs["pos"]), gt=up(hs["pos_gt"]), T_w=up(hs["T_w"][0].reshape(-1, 16)), time=up(hs["time"]),
                         T_oc=None if hs["T_oc"] is None else up(hs["T_oc"].reshape(-1, 16)),
                         desc=p[r].desc_dev[torch.from_numpy(keep[r].astype(np.int64)).to(dev)].contiguous() if d else None))

    # ---- pass 1 on the device: one enqueue, one synchronisation, the pair list and the dense matrices back ----
    g = _gate_buffers(torch, dev, n0, n1)
    gp = grid_gate_params(sm_params.submap_radius, sm_io.skip_distance, d, sm_params.submap_descriptor_thresh if d else 0.0,
                          sm_params.single_robot_lc, sm_params.single_robot_lc_time_thresh)
    if stacked:
        gp.desc_thresh = float(sm_params.submap_descriptor_thresh)
        masks = [q.frame_mask[torch.from_numpy(k.astype(np.int64)).to(dev)].contiguous() for q, k in zip(p, keep)]     # rows gathered on the device
    if aabb_mode:                                            # the boxes of the non-empty submaps of either pool: slot rows and counts gathered per kept submap
        boxes = [torch.empty((len(k), 6), dtype=torch.float64, device=dev) for k in keep]
        counts = [up(q.count[k].astype(np.int32)) for q, k in zip(p, keep)]
        slots = [q.pool if len(k) == len(q.count) else
                 q.pool.reshape(len(q.count), q.cap, -1)[torch.from_numpy(k.astype(np.int64)).to(dev)].reshape(len(k) * q.cap, -1).contiguous() for q, k in zip(p, keep)]
    wait_torch()                                             # the uploads are in place before the library's stream reads them
    if aabb_mode:
        for r in range(2):
            ctx.submap_boxes_dev(len(keep[r]), int(slots[r].shape[1]), p[r].cap, slots[r].data_ptr(), counts[r].data_ptr(), side[r]["T_oc"].data_ptr(),
                                 boxes[r].data_ptr())
    if stacked:                                              # similarity first, then the gate that reads it: both on the context's stream
        fd = [q.frame_desc_dev for q in p]
        ctx.stacked_sim_dev(int(fd[0].shape[1]), int(fd[0].shape[0]), ptr(fd[0]), n0, ptr(masks[0]), int(fd[1].shape[0]), ptr(fd[1]), n1, ptr(masks[1]),
                            g["sim"].data_ptr())
    gate_args = (gp, n0, n1, ptr(side[0]["pos"]), ptr(side[0]["T_w"]), ptr(side[1]["pos"]), ptr(side[1]["T_w"]), *[t.data_ptr() for t in g.values()])
    gate_kw = dict(time0_ptr=ptr(side[0]["time"]), time1_ptr=ptr(side[1]["time"]), pos_gt0_ptr=ptr(side[0]["gt"]), pos_gt1_ptr=ptr(side[1]["gt"]))
    desc_kw = dict(desc0_ptr=ptr(side[0]["desc"]), desc1_ptr=ptr(side[1]["desc"]))
    if aabb_mode:
        ctx.grid_gate_aabb_dev(*gate_args, box0_ptr=boxes[0].data_ptr(), box1_ptr=boxes[1].data_ptr(), sim_in_ptr=g["sim"].data_ptr() if stacked else None,
                               **gate_kw, **desc_kw)
    elif stacked:
        ctx.grid_gate_sim_dev(*gate_args, **gate_kw)
    else:
        ctx.grid_gate_dev(*gate_args, **gate_kw, **desc_kw)
    ctx.sync()
    B = int(g["n_todo"].cpu().numpy()[0])
    pairs = g["pairs"][:B].cpu().numpy().astype(np.int64)
    h = {k: g[k].cpu().numpy() for k in ("dist", "flags", "yaw", "sim", "T_ij")}
    nearby, todo = _pass1_block(M, h, 0, n0 * n1, n0, n1, pairs, "roman_grid_gate_dev: the compact pair list is not the TODO pairs in row-major order")
    if B == 0:
        return M.results(lc_edges=M.empty_edges(), hypotheses=None if num_solutions is None else {})

    # ---- the hot path over the resident pools: offsets and counts from the pools, the batch in chunks, then the tail ----
    batch, pool = p[0].grid_batch(p[1], mask=todo)
    kmax = batch.kmax()                                      # (of the unreduced sizes: still a bound after the removal)
    if shared:
        ids_dev = p[0].ids_dev if p[0] is p[1] else torch.cat([p[0].ids_dev, p[1].ids_dev])
        pool, *prob = _drop_shared_over_pool(torch, ctx, pool, ids_dev, batch.off1, batch.n1, batch.off2, batch.n2, np.arange(B), wait_torch)
        batch = AlignmentBatch(np.broadcast_to(np.float64(0.0), tuple(pool.shape)), *prob, pair_index=batch.pair_index)
    res, per_pair = _register_over_pool(torch, ctx, registration, sm_params, sm_io, pool, batch, kmax, g, B, up(frames[0].reshape(-1, 16)),
                                        up(frames[1].reshape(-1, 16)), wait_torch, num_solutions)
    out = M.results([per_pair] * B, _records_into_results(M, res, pairs[:, 0], pairs[:, 1], nearby))
    out.hypotheses = _hypotheses_of(res, pairs[:, 0], pairs[:, 1])
    return out


def _one_storage(torch, parts):
    """The tensors `parts` as ONE tensor without a copy, where they allow it: each contiguous, all in the same storage, each
    starting where the one in front of it ends (the pools build_session_pools leaves are such row ranges) -> a
    view of that storage over all their rows, or None — a gap, another order, separately allocated tensors, a missing one —, and
    the caller concatenates as before."""
    if len(parts) < 2 or any(q is None or not q.is_contiguous() for q in parts):
        return None
    first = parts[0]
    base, at, tail = first.untyped_storage().data_ptr(), first.data_ptr(), tuple(first.shape[1:])
    for q in parts:
        if q.untyped_storage().data_ptr() != base or q.data_ptr() != at or tuple(q.shape[1:]) != tail or q.dtype != first.dtype:
            return None
        at += q.numel() * q.element_size()
    shape = (sum(int(q.shape[0]) for q in parts),) + tail
    stride = tuple(int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))
    return first.as_strided(shape, stride, first.storage_offset())


def _session_setup(sm_params, pools, robot_pairs, sm_io, registration, gt_poses, num_solutions):
    """The arguments of a session call made whole, and every refusal that needs no context, in submap_align_session's order
    -> the record every later stage reads: the arguments (sm_io and registration defaulted), p (the pools), R, gt_poses (R
    entries), blocks, aabb_mode, mode, stacked, d (the gate's descriptor length), selfs (the robots with a self block), keep and
    counts (per robot: the pool indices of its non-empty submaps, and how many) and way (the tail of every refusal)."""
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    way = " (not in the session call: use submap_align_pools per robot pair)"
    p = list(pools)
    R = len(p)
    gt_poses = [None] * R if gt_poses is None else list(gt_poses)
    blocks = [(r, s) for r in range(R) for s in range(r, R)] if robot_pairs is None else [(int(r), int(s)) for r, s in robot_pairs]
    if len(gt_poses) != R:
        raise ValueError("gt_poses must hold one entry per pool" + way)
    if any(not (0 <= r < R and 0 <= s < R) for r, s in blocks) or len(set(blocks)) != len(blocks):
        raise ValueError("robot_pairs must name pools by index, each pair once" + way)
    if num_solutions is not None:                            # (submap_align_pools' three for K hypotheses per pair)
        _mno_refusals(registration, p, blocks, num_solutions, way)
    if isinstance(registration, RansacReg) and R:            # (submap_align_pools' four, in its order: in front of everything that makes a HIP context)
        _ransac_refusals(registration, p, way)
    if _device_prefilter(registration) and R:                # (and its four for a device-prefilter plugin)
        _prune_refusals(registration, p, way)
    aabb_mode = bool(sm_params.force_fill_submaps or sm_params.submap_radius is None)
    if aabb_mode and _no_device(registration, p):            # (the boxes are reduced from the resident rows: as for a RansacReg, host rows need a context of the caller's)
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes of the resident rows: the registration has no context set "
                         "and the pools are host tensors: no device to run on" + way)
    mode = sm_params.submap_descriptor
    _descriptor_refusals(registration, p, mode, way)
    if R and any(int(q.pool.shape[1]) != int(p[0].pool.shape[1]) for q in p):
        raise ValueError("the pools have different row widths" + way)
    d = _descriptor_dim(p, mode, "the pools", way)
    selfs = sorted({r for r, s in blocks if r == s})
    if any(p[r].ids_dev is None for r in selfs):
        raise ValueError("a self block drops the segments both submaps hold: its pool must have kept its ids on the device (SubmapPool.ids_dev, "
                         "as build_submap_pool leaves it)" + way)
    keep = [q.nonempty for q in p]
    return SimpleNamespace(sm_params=sm_params, sm_io=sm_io, registration=registration, num_solutions=num_solutions, p=p, R=R, gt_poses=gt_poses,
                           blocks=blocks, aabb_mode=aabb_mode, mode=mode, stacked=mode == 'stacked_frame_descriptors', d=d, selfs=selfs, keep=keep,
                           counts=np.array([len(k) for k in keep], dtype=np.int64), way=way)


def _session_views(s):
    """Per robot (O(S), host): the block submap_align_pools runs per side, with the reads of the pair loop it would see.  A pose
    read `n` times (n: the partner's submaps) usually sits at a fixed point after a read or two, and the robot then has ONE set of
    arrays for all its blocks; where flattening a pose alternates between two neighbouring values, its reference transform
    depends on n, and the robot enters the tables once per distinct outcome (a "view": same pool rows, own T_w and edge frames,
    own T_oc in bounding-box mode).  -> views [(robot, host arrays or None)], vblocks (per block: its two views), vcount (per
    view: its submaps) and runtime.session_tables over them (sub_off, blocks, pair_off, tile_off)."""
    from ..runtime import session_tables
    p, blocks, counts = s.p, s.blocks, s.counts
    views, view_of = [], {}
    for r in range(s.R):
        reads = sorted({int(counts[b if a == r else a]) for a, b in blocks if r in (a, b)})
        mine = []
        live_reads = [n for n in reads if n > 0] if counts[r] else []       # (an empty block: the robot only needs a place in the tables)
        all_ = _pool_side_host(p[r], s.gt_poses[r], s.gt_poses[r] is not None, live_reads, s.aabb_mode) if live_reads else None
        for k, n in enumerate(live_reads):
            hs = dict(all_, T_w=[all_["T_w"][k]], frames=all_["frames"][k])
            key = hs["T_w"][0].tobytes() + hs["frames"][0].tobytes() + hs["frames"][1].tobytes() + (hs["T_oc"].tobytes() if s.aabb_mode else b"")
            same = [v for v, kk in mine if kk == key]
            if not same:
                views.append((r, hs)); mine.append((len(views) - 1, key))
            view_of[(r, n)] = same[0] if same else len(views) - 1
        if reads and not mine:                               # only in empty blocks: zeros stand in (never read)
            views.append((r, None)); mine.append((len(views) - 1, b""))
        for n in reads:
            view_of.setdefault((r, n), mine[0][0])
    vcount = np.array([counts[r] for r, _ in views], dtype=np.int64)
    vblocks = [(view_of[(a, int(counts[b]))], view_of[(b, int(counts[a]))]) for a, b in blocks]
    return views, vblocks, vcount, session_tables(vcount, [(va, vb, a == b) for (va, vb), (a, b) in zip(vblocks, blocks)])


def _session_block_results(s):
    """-> prm (per block: the parameters with its own single_robot_lc), Ms (its fresh _GridResults over the non-empty submaps) and
    result_of(b, M, timing, edges, hyps): block b's SubmapAlignResults out of M, with its own gt_available."""
    def result_of(b, M, timing=(), edges=None, hyps=None):
        io = copy.copy(s.sm_io); io.gt_available = (s.gt_poses[s.blocks[b][0]] is not None, s.gt_poses[s.blocks[b][1]] is not None)
        M.sm_io = io
        return M.results(timing, edges, hyps if s.num_solutions is None or hyps is not None else {})
    prm = [copy.copy(s.sm_params) for _ in s.blocks]
    for q, (a, b) in zip(prm, s.blocks):
        q.single_robot_lc = (a == b)
    return prm, [_GridResults(prm[k], s.sm_io, int(s.counts[a]), int(s.counts[b])) for k, (a, b) in enumerate(s.blocks)], result_of


def _session_context(s, gate_entry):
    """The registration's context, and the refusals that ask the context itself (as submap_align_pools does, they come once it
    exists).  `gate_entry`: the gate the caller enqueues, 'session_gate_dev' (with session_gate_aabb_dev beside it for the
    bounding-box gate) or 'session_gate_list_dev' (which serves the boxes itself).  -> the context."""
    ctx, way = s.registration._context(), s.way
    if s.num_solutions is not None and not hasattr(ctx, "mno_lc_tail_dev"):
        raise ValueError("the context has no roman_mno_lc_tail_dev" + way)
    if s.selfs and not hasattr(ctx, "shared_reduce_dev"):
        raise ValueError("self blocks need a context with roman_shared_reduce_dev" + way)
    if not hasattr(ctx, gate_entry):
        raise ValueError(f"the context has no roman_{gate_entry}" + way)
    if s.stacked and not hasattr(ctx, "session_stacked_sim_dev"):
        raise ValueError("the context has no roman_session_stacked_sim_dev" + way)
    box_calls = ["session_boxes_dev"] + (["session_gate_aabb_dev"] if gate_entry == "session_gate_dev" else [])
    if s.aabb_mode and not all(hasattr(ctx, name) for name in box_calls):
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes: the context has no " +
                         " / ".join("roman_" + name for name in box_calls) + way)
    if s.aabb_mode and any(int(q.table.point_dim) != 3 for q in s.p):
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes, and pools of dim 2: their rows hold no z" + way)
    return ctx


def _session_uploads(torch, s, views, sub_off, blk, pair_off):
    """The session-wide arrays of the gate on the pools' device -> a record: dev, wait_torch / up / ptr (`_plumbing`), lv (the views
    that hold submaps, in table order), cat(get, width) (a host array per view, concatenated over lv), FLh / FRh (the edge frames
    over all submaps, host), rows_of (per live robot: its non-empty submaps as a device index) and t, the device tables by name
    (the caller adds the one its own gate reads: tile_off or list).  Stacked descriptors: ONE frame table (fdesc) and ONE block
    of mask words (fmask) for the session — every live robot's frame descriptors once and the mask rows of its non-empty submaps
    (gathered on the device) once, whatever number of views it has: the views of a robot name the same frames and the same
    words — with frame_lo, frame_n, mask_off per view, host here and device in t."""
    p, counts, gt_poses = s.p, s.counts, s.gt_poses
    dev = p[0].pool.device
    wait_torch, up, ptr = _plumbing(torch, dev)
    lv = [(r, hs) for r, hs in views if counts[r]]
    cat = lambda get, width: np.concatenate([np.zeros((int(counts[r]),) + width) if hs is None else np.asarray(get(hs)).reshape((-1,) + width) for r, hs in lv])
    any_gt = any(gt_poses[r] is not None for r, _ in lv)
    pos_gt = None
    if any_gt:
        pos_gt = np.concatenate([np.full((int(counts[r]), 3), np.nan) if (hs is None or hs["pos_gt"] is None) else hs["pos_gt"] for r, hs in lv])
    rows_of = {r: torch.from_numpy(s.keep[r].astype(np.int64)).to(dev) for r in {r for r, _ in lv}} if s.d or s.stacked else {}
    t = dict(pos=up(cat(lambda hs: hs["pos"], (3,))), gt=up(pos_gt),
             has=up(np.array([gt_poses[r] is not None for r, _ in views], dtype=np.int32)) if any_gt else None,
             T_w=up(cat(lambda hs: hs["T_w"][0], (16,))), time=up(cat(lambda hs: hs["time"], ())), sub_off=up(sub_off), blocks=up(blk),
             pair_off=up(pair_off), desc=torch.cat([p[r].desc_dev[rows_of[r]] for r, _ in lv]).contiguous() if s.d else None)
    u = SimpleNamespace(dev=dev, wait_torch=wait_torch, up=up, ptr=ptr, lv=lv, cat=cat, FLh=cat(lambda hs: hs["frames"][0], (16,)),
                        FRh=cat(lambda hs: hs["frames"][1], (16,)), rows_of=rows_of, t=t)
    if s.stacked:
        live_f = sorted(rows_of)
        u.fdesc = _one_storage(torch, [p[r].frame_desc_dev for r in live_f])       # (grow_session_pools' frame tables are row ranges of one storage, §4.23)
        if u.fdesc is None:
            u.fdesc = p[live_f[0]].frame_desc_dev if len(live_f) == 1 else torch.cat([p[r].frame_desc_dev for r in live_f], dim=0)
        u.fmask = torch.cat([p[r].frame_mask[rows_of[r]].reshape(-1) for r in live_f]).contiguous()
        nfr = {r: int(p[r].frame_desc_dev.shape[0]) for r in live_f}
        flo = dict(zip(live_f, np.concatenate([[0], np.cumsum([nfr[r] for r in live_f])]).astype(np.int64).tolist()))
        mof = dict(zip(live_f, np.concatenate([[0], np.cumsum([int(counts[r]) * ((nfr[r] + 63) // 64) for r in live_f])]).astype(np.int64).tolist()))
        u.frame_lo = np.array([flo.get(r, 0) for r, _ in views], dtype=np.int32)
        u.frame_n = np.array([nfr.get(r, 0) for r, _ in views], dtype=np.int32)
        u.mask_off = np.array([mof.get(r, 0) for r, _ in views], dtype=np.int64)
        t.update(frame_lo=up(u.frame_lo), frame_n=up(u.frame_n), mask_off=up(u.mask_off))
    return u


def _session_pool(torch, s, lv):
    """ONE pool for the session — every live robot's rows once, whatever the number of its views (lv: the views that hold
    submaps) — and per GLOBAL submap index (the gate's, as sub_off orders them) its first row and its rows
    -> (pool, sm_row int64, sm_cnt int32).  Pools of ONE build (build_session_pools) are read in place (`_one_storage`); any other
    list is concatenated: a copy of every row, so a caller that may not need the pool asks late."""
    p = s.p
    live = sorted({r for r, _ in lv})
    pool = _one_storage(torch, [p[r].pool for r in live])
    if pool is None:
        pool = p[live[0]].pool if len(live) == 1 else torch.cat([p[r].pool for r in live], dim=0)
    row0 = dict(zip(live, np.concatenate([[0], np.cumsum([int(p[r].pool.shape[0]) for r in live])]).astype(np.int64).tolist()))
    return (pool, np.concatenate([row0[r] + p[r].offsets()[0] for r, _ in lv]).astype(np.int64),
            np.concatenate([p[r].offsets()[1] for r, _ in lv]).astype(np.int32))


def _session_pass1_front(torch, ctx, s, u, sub_off, blk, pair_off, n_out, one_pool, sim_total=None, lst=None):
    """What pass 1 of a session enqueues in front of its gate -> (g, gp, gate_kw): g the gate's output buffers, `n_out` entries each
    (todo_off: one per block and one), gp its parameters, gate_kw its optional pointers.  Behind wait_torch(), on the context's
    stream: for the bounding-box gate ONE session_boxes_dev over `one_pool` (`_session_pool`'s: rows by offset and count, no
    gather into slots; a view's own T_odom_center — two views of a robot: the same rows, two box sets) into t["box"]; for
    stacked descriptors session_stacked_sim_dev over whole blocks — into g["sim"], or with `sim_total` into a dense buffer of
    that many entries, t["dense_sim"] —, which gate_kw hands to the gate as sim_in_ptr.  `lst` (with sim_total; t["list"] is its
    device copy): the pairs the gate will read.  Where the list leaves a pair out and the context has
    session_stacked_sim_list_dev, ONE such call writes the listed entries of t["dense_sim"] and nothing else;
    a full list, a first call and a context without the entry take the whole-block call."""
    f64, i32 = torch.float64, torch.int32
    sm_params, t, up, ptr, dev, n = s.sm_params, u.t, u.up, u.ptr, u.dev, n_out
    if s.aabb_mode:
        pool, sm_row, sm_cnt = one_pool
        t.update(row0=up(sm_row), count=up(sm_cnt), T_oc=up(u.cat(lambda hs: hs["T_oc"], (16,))), box=torch.empty((len(sm_cnt), 6), dtype=f64, device=dev))
    g = dict(dist=torch.empty(n, dtype=f64, device=dev), flags=torch.empty(n, dtype=i32, device=dev), yaw=torch.empty(n, dtype=f64, device=dev),
             sim=torch.empty(n, dtype=f64, device=dev), T_ij=torch.empty((n, 16), dtype=f64, device=dev),
             pairs=torch.empty((n, 2), dtype=i32, device=dev), T_ref=torch.empty((n, 16), dtype=f64, device=dev),
             enable=torch.empty(n, dtype=i32, device=dev), todo_off=torch.zeros(len(s.blocks) + 1, dtype=i32, device=dev))
    gp = grid_gate_params(sm_params.submap_radius, s.sm_io.skip_distance, s.d, sm_params.submap_descriptor_thresh if s.d else 0.0,
                          False, sm_params.single_robot_lc_time_thresh)
    gate_kw = dict(time_ptr=ptr(t["time"]), desc_ptr=ptr(t["desc"]), pos_gt_ptr=ptr(t["gt"]), has_gt_ptr=ptr(t["has"]))
    if s.stacked and sim_total is not None:
        t["dense_sim"] = torch.empty(sim_total, dtype=f64, device=dev)
    u.wait_torch()                                           # the uploads are in place before the library's stream reads them
    if s.aabb_mode:
        ctx.session_boxes_dev(len(sm_cnt), int(pool.shape[1]), pool.data_ptr(), ptr(t["row0"]), ptr(t["count"]), ptr(t["T_oc"]), ptr(t["box"]))
    if s.stacked:                                            # similarity first, then the gate that reads it: both on the context's stream
        gp.desc_thresh = float(sm_params.submap_descriptor_thresh)
        sim = (g["sim"] if sim_total is None else t["dense_sim"]).data_ptr()
        tables = (u.frame_lo, u.frame_n, u.mask_off, sub_off, blk, pair_off)
        table_ptrs = [ptr(t[k]) for k in ("frame_lo", "frame_n", "mask_off", "sub_off", "blocks", "pair_off")]
        if sim_total is not None and lst is not None and len(lst) < sim_total and hasattr(ctx, "session_stacked_sim_list_dev"):
            ctx.session_stacked_sim_list_dev(int(u.fdesc.shape[1]), int(u.fdesc.shape[0]), ptr(u.fdesc), ptr(u.fmask), *tables, lst, *table_ptrs, ptr(t["list"]), sim)
        else:
            ctx.session_stacked_sim_dev(int(u.fdesc.shape[1]), int(u.fdesc.shape[0]), ptr(u.fdesc), ptr(u.fmask), *tables, *table_ptrs, sim)
        gate_kw["sim_in_ptr"] = sim
    return g, gp, gate_kw


def _session_register(torch, ctx, s, u, gpairs, todo_off, one_pool, g):
    """Every TODO pair of every block as a problem of ONE batch over `one_pool` (`_session_pool`'s), in the compact order pass 1
    left in g: `gpairs` (B, 2) global submap indices, block b's at [todo_off[b], todo_off[b + 1]).  The problems of the self
    blocks lose the segments both submaps hold; then `_register_over_pool`.  For a RansacReg too the problems of ALL blocks go
    in one batch: the seed is one per batch and a problem's draws do not depend on its place in it,
    so a block equals its own submap_align_pools.  -> (parts, per_pair): one LoopClosureResult per block, its accepted indices
    block-local, with `hypotheses` when num_solutions is set."""
    p = s.p
    pool, sm_row, sm_cnt = one_pool
    prob = sm_row[gpairs[:, 0]], sm_cnt[gpairs[:, 0]], sm_row[gpairs[:, 1]], sm_cnt[gpairs[:, 1]]
    kmax = int(max(1, np.max(np.minimum(prob[1], prob[3]))))    # (of the unreduced sizes: still a bound after the removal)
    of_self = np.concatenate([np.full(int(todo_off[b + 1] - todo_off[b]), a == c, dtype=bool) for b, (a, c) in enumerate(s.blocks)])
    sel = np.nonzero(of_self)[0]
    if len(sel):
        live = sorted({r for r, _ in u.lv})
        ids_dev = _one_storage(torch, [p[r].ids_dev for r in live])
        if ids_dev is None or int(ids_dev.shape[0]) != int(pool.shape[0]):
            ids_dev = torch.cat([p[r].ids_dev if p[r].ids_dev is not None else torch.zeros(int(p[r].pool.shape[0]), dtype=torch.int64, device=u.dev) for r in live])
        pool, *prob = _drop_shared_over_pool(torch, ctx, pool, ids_dev, *prob, sel, u.wait_torch)
    batch = AlignmentBatch(np.broadcast_to(np.float64(0.0), tuple(pool.shape)), prob[0].astype(np.int64), prob[1].astype(np.int32), prob[2].astype(np.int64),
                           prob[3].astype(np.int32), pair_index=gpairs)
    res, per_pair = _register_over_pool(torch, ctx, s.registration, s.sm_params, s.sm_io, pool, batch, kmax, g, len(gpairs), u.up(u.FLh), u.up(u.FRh),
                                        u.wait_torch, s.num_solutions)
    parts = []
    acc = np.asarray(res.accepted, dtype=np.int64)
    for b in range(len(s.blocks)):
        lo, hi = int(todo_off[b]), int(todo_off[b + 1])
        part = LoopClosureResult(res.assoc[lo:hi], res.T[lo:hi], res.status[lo:hi], res.stats[lo:hi], res.records[lo:hi],
                                 acc[(acc >= lo) & (acc < hi)] - lo)
        if s.num_solutions is not None:
            part.hypotheses = res.hypotheses[lo:hi]
        parts.append(part)
    return parts, per_pair


def submap_align_session(sm_params, pools, robot_pairs=None, sm_io: Optional[SubmapAlignIO] = None, registration=None,
                         gt_poses=None, num_solutions=None) -> Dict[Tuple[int, int], SubmapAlignResults]:
    """The robot-pair loop of the reference's driver [REF demo/demo.py:138-161] in ONE call: `pools` is a list of R
    device-resident SubmapPool, `robot_pairs` the blocks (r, s) to align — default: every r <= s in the driver's order.  -> {(r, s):
    SubmapAlignResults}, each equal to what submap_align_pools(p, [pools[r], pools[s]], ...) returns for that block alone with
    single_robot_lc = (r == s), as [REF demo/demo.py:160] sets it.  sm_params.single_robot_lc is IGNORED.

    gt_poses[r] follows submap_align_pools; a block's sm_io.gt_available is (gt_poses[r] is not None, gt_poses[s] is not None).
    `sm_io` is shared by all blocks (every result carries a copy with its own gt_available); the caller names the output files
    when it calls the writers on each result.

    Per robot the O(S) host block runs once per distinct outcome of the pair loop's pose reads (as a rule: once) and goes up
    once; pass 1 of all blocks is one roman_session_gate_dev, one
    synchronisation and one read-back; every TODO pair of every block is a problem of ONE batch over the concatenated pools
    (self blocks lose the segments both submaps hold through one roman_shared_reduce_dev over their problems); one
    issue_chunked, one join, one roman_lc_tail_dev with the frames tabled over all submaps of the session.

    Pools that are consecutive row ranges of ONE storage, in list order — what build_session_pools leaves — are
    read in place: the batch and the shared-segment removal run over a view of that storage, nothing is concatenated, and every
    block is what it is over separately built pools.  Any other list (separately built pools, a gap, another order) is
    concatenated as before (`_one_storage`).

    'stacked_frame_descriptors' (pools built with it): every live robot's frame descriptors go ONCE into the
    session's frame table and the mask rows of its non-empty submaps once into one block of words, whatever number of views the
    robot has; roman_session_stacked_sim_dev writes the similarity of every pair of every block and roman_session_gate_sim_dev
    behind it, on the same stream, gates on it.  similarity_mat per block is what the device computed.

    force_fill_submaps / no submap_radius: the gate is aabb_intersects over segments_as_global_points
    [REF roman/align/submap_align.py:101-103].  ONE roman_session_boxes_dev reduces every submap of every view to its box, straight
    from the concatenated pools the batch reads anyway (rows by offset and count, a view's own T_odom_center — the ground-truth
    pose where gt_poses[r] is given); roman_session_gate_aabb_dev is the gate, behind roman_session_stacked_sim_dev for stacked
    descriptors — all on the context's stream, with the one synchronisation of the radius mode.  Pools built by
    build_submap_pool(fill=...) and radius-mode pools are served alike, in one session too.

    A RansacReg (method='ransac'): pass 1 and the shared-segment removal of the self blocks unchanged, then
    the problems of ALL blocks through one `_ransac_lc_over_pool` (roman_ransac_lc_batch_dev and the tail, chunked by
    RANSAC_ASSOC_CHUNK_BYTES) in place of issue_chunked, join and the tail.  The seed is one per batch and a problem's result does
    not depend on its place in it: every block equals submap_align_pools with the same registration.  Both together work too.

    method='clipper+prune' with the device-prefilter plugin (DistRegWithPruning.on_device()) over pools built
    with it: a CLIPPER method like any other — the problems of all blocks in the one issue_chunked, self blocks through the one
    roman_shared_reduce_dev with their full-width rows —, every block equal to submap_align_pools with the same plugin.

    Not covered — ValueError before any context is made; submap_align_pools per robot pair is the way: a plugin whose prefilter
    runs on the host (DistRegWithPruning.on_device() is the one that is served), for a device-prefilter plugin the four things
    submap_align_pools refuses for it (semantics_dim unset, row width, desc_dim, a table packed by another registration), pools of
    different row width or descriptor length, pools not built with the frame-descriptor mode asked for, a self
    block over a pool without ids_dev, and whatever submap_align_pools refuses for a pool — for a RansacReg its four (pools of
    dim 2, a `cap` above ROMAN_RANSAC_MAX_OBJECTS, host-tensor pools while the registration has no context set, a context without
    roman_ransac_lc_batch_dev), in its order.  The bounding-box gate over host-tensor pools while the registration has no context
    set is refused there as well: there is no device the rows could be reduced on.  The other refusals ask the context itself and
    so come after it exists, as in submap_align_pools: a context without roman_session_gate_dev, one without
    roman_session_stacked_sim_dev for stacked descriptors, one without roman_shared_reduce_dev when the list holds a self block,
    and for the bounding-box gate a context without roman_session_boxes_dev / roman_session_gate_aabb_dev, or pools of dim 2
    (their rows hold no z)."""
    import torch
    sess = _session_setup(sm_params, pools, robot_pairs, sm_io, registration, gt_poses, num_solutions)
    blocks, counts = sess.blocks, sess.counts
    views, vblocks, _, (sub_off, blk, pair_off, tile_off) = _session_views(sess)
    # ---- the refusals that need no context are behind us: the tables, the context, the uploads ----
    _, Ms, result_of = _session_block_results(sess)
    total, nb = int(pair_off[-1]), len(blocks)
    if total == 0:
        return {blocks[b]: result_of(b, Ms[b], edges=Ms[b].empty_edges()) for b in range(nb)}
    ctx = _session_context(sess, "session_gate_dev")
    u = _session_uploads(torch, sess, views, sub_off, blk, pair_off)
    t, ptr = u.t, u.ptr
    t["tile_off"] = u.up(tile_off)

    # ---- pass 1 of all blocks on the device: one enqueue, one synchronisation, one read-back.  The bounding-box gate reads the
    # ONE pool now; the radius gate leaves it until a pair is TODO (a list of separately built pools is copied into it) ----
    one_pool = _session_pool(torch, sess, u.lv) if sess.aabb_mode else None
    g, gp, gate_kw = _session_pass1_front(torch, ctx, sess, u, sub_off, blk, pair_off, total, one_pool)
    gate_args = (gp, sub_off, blk, pair_off, tile_off, ptr(t["sub_off"]), ptr(t["blocks"]), ptr(t["pair_off"]), ptr(t["tile_off"]), ptr(t["pos"]), ptr(t["T_w"]),
                 *[g[k].data_ptr() for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off")])
    if sess.aabb_mode:
        ctx.session_gate_aabb_dev(*gate_args, ptr(t["box"]), **gate_kw)
    else:
        ctx.session_gate_dev(*gate_args, **gate_kw)
    ctx.sync()
    todo_off = g["todo_off"].cpu().numpy().astype(np.int64)
    B = int(todo_off[-1])
    gpairs = g["pairs"][:B].cpu().numpy().astype(np.int64)
    h = {k: g[k].cpu().numpy() for k in ("dist", "flags", "yaw", "sim", "T_ij")}
    nearby, local = [], []
    for b, (r, s) in enumerate(blocks):
        n0, n1 = int(counts[r]), int(counts[s])
        lp_ = gpairs[todo_off[b]:todo_off[b + 1]] - np.array([sub_off[vblocks[b][0]], sub_off[vblocks[b][1]]], dtype=np.int64)
        near, _ = _pass1_block(Ms[b], h, int(pair_off[b]), int(pair_off[b + 1]), n0, n1, lp_,
                               f"roman_session_gate_dev: the compact pair list of block {blocks[b]} is not its TODO pairs in row-major order")
        nearby.append(near); local.append(lp_)
    if B == 0:
        return {blocks[b]: result_of(b, Ms[b], edges=Ms[b].empty_edges()) for b in range(nb)}

    # ---- ONE batch over the ONE pool, then the records and the accepted list per block, with block-local indices ----
    parts, per_pair = _session_register(torch, ctx, sess, u, gpairs, todo_off, one_pool or _session_pool(torch, sess, u.lv), g)
    out = {}
    for b, part in enumerate(parts):
        ti, tj = local[b][:, 0], local[b][:, 1]
        edges = _records_into_results(Ms[b], part, ti, tj, nearby[b]) if len(ti) else Ms[b].empty_edges()
        out[blocks[b]] = result_of(b, Ms[b], [per_pair] * len(ti), edges, _hypotheses_of(part, ti, tj))
    return out


# ---------------------------------------------------------------------------------------------
# a session that GROWS: only the pairs a new or changed submap touches
# ---------------------------------------------------------------------------------------------
class SessionAlignState:
    """What submap_align_session_update keeps between two steps of one session: the call it was made for, per robot the submaps
    it saw and the bytes of their host-side inputs, and every block's results.  Empty until the first call."""

    def __init__(self):
        self.key = None              # robot_pairs, method, descriptor mode, gate, ground truth, num_solutions: a state serves ONE kind of call
        self.n_pool = None           # per robot: the submaps of its pool, empty ones included
        self.keep = None             # per robot: the pool indices of its non-empty submaps
        self.seen = None             # per (block, side): uint8 (n, bytes) — the host-side inputs of every non-empty submap as that block read them
        self.results = None          # {(r, s): SubmapAlignResults} as returned last
        self.listed = 0              # pairs the last call listed, and what the full grids hold (for the caller's accounting)
        self.total = 0
        self.seconds = {}            # the last call's wall time by part: 'host' (the per-robot block, the touched set, the carry-over), 'gate' (uploads,
                                     # pass 1, its synchronisation and read-back), 'register' (the batch, the tail and the records)


_MATRICES = ("robots_nearby_mat", "clipper_angle_mat", "clipper_dist_mat", "clipper_num_associations", "similarity_mat", "submap_yaw_diff_mat",
             "T_ij_mat", "T_ij_hat_mat")


def _carry_over(M, old, old_keep, new_keep):
    """The stored results `old` of a block into the fresh matrices `M`, re-indexed through the pool indices of the non-empty
    submaps (old_keep / new_keep: one array per side) -> (edges, hypotheses) re-indexed the same way; a submap that is gone
    takes its entries with it."""
    where = [{int(s): k for k, s in enumerate(nk)} for nk in new_keep]
    to_new = [np.array([where[a].get(int(s), -1) for s in ok], dtype=np.int64) for a, ok in enumerate(old_keep)]
    src = [np.nonzero(t >= 0)[0] for t in to_new]
    dst = [t[t >= 0] for t in to_new]
    appended = all(len(ok) <= len(nk) and np.array_equal(ok, nk[:len(ok)]) for ok, nk in zip(old_keep, new_keep))
    if appended and len(src[0]) and len(src[1]):             # the usual step: the old grid is the top left corner of the new one
        a, b = len(old_keep[0]), len(old_keep[1])
        for name in _MATRICES:
            if getattr(old, name) is not None:
                getattr(M, name)[:a, :b] = getattr(old, name)
        extra = len(new_keep[1]) - b
        for i in range(a):
            M.associated_objs_mat[i] = old.associated_objs_mat[i] + [[] for _ in range(extra)]
    elif len(src[0]) and len(src[1]):
        for name in _MATRICES:
            if getattr(old, name) is not None:
                getattr(M, name)[np.ix_(dst[0], dst[1])] = getattr(old, name)[np.ix_(src[0], src[1])]
        back = np.full(len(new_keep[1]), -1, dtype=np.int64)        # new column -> old column
        back[dst[1]] = src[1]
        back = back.tolist()
        for i_old, i_new in zip(src[0].tolist(), dst[0].tolist()):
            row = old.associated_objs_mat[i_old]
            M.associated_objs_mat[i_new] = [row[j] if j >= 0 else [] for j in back]
    edges = None
    if old.lc_edges is not None:
        pr = np.asarray(old.lc_edges["pairs"], dtype=np.int64).reshape(-1, 2)
        pr = np.stack([to_new[0][pr[:, 0]], to_new[1][pr[:, 1]]], axis=1) if len(pr) else pr
        ok = (pr >= 0).all(axis=1)
        edges = dict(pairs=pr[ok], t=np.asarray(old.lc_edges["t"]).reshape(-1, 3)[ok], q=np.asarray(old.lc_edges["q"]).reshape(-1, 4)[ok])
    hyps = None
    if old.hypotheses is not None:
        hyps = {(int(to_new[0][i]), int(to_new[1][j])): h for (i, j), h in old.hypotheses.items() if to_new[0][i] >= 0 and to_new[1][j] >= 0}
    return edges, hyps


def submap_align_session_update(state, sm_params, pools, touched=None, robot_pairs=None, sm_io: Optional[SubmapAlignIO] = None, registration=None,
                                gt_poses=None, num_solutions=None) -> Dict[Tuple[int, int], SubmapAlignResults]:
    """submap_align_session for a session that GROWS: `state` (a SessionAlignState, empty before the first call)
    keeps every block's results, and a call gates and registers only the pairs with a TOUCHED submap on either side — one
    roman_session_gate_list_dev over the pair list, one batch over the pools, the shared-segment removal and the tail as in
    submap_align_session.  -> {(r, s): SubmapAlignResults} over EVERY block, equal to submap_align_session(sm_params, pools, ...)
    over the same pools (only timing_list differs: it holds the pairs registered in this call).  A first call is the full call.

    Between two calls a pool may only grow by APPENDING submaps: submap s of robot r stays submap s (one that was empty may fill).
    touched[r] (bool over robot r's pool submaps, or None) flags the submaps whose rows, ids or frames the caller changed — as
    the last submap of the step before, whose t_hi moves when a successor arrives.  The call adds on its own: every submap beyond
    the robot's earlier count; every submap that was empty; and every submap whose host-side inputs differ, by bytes, from what the
    state recorded for ANY block the robot takes part in — centre, ground-truth centre, time, and what depends on the pose as the
    pair loop leaves it: reference pose, edge frames, the box pose of the bounding-box gate.  The last three can change without
    the caller's doing: what the pair loop reads of a pose can depend on the partner's number of submaps, so
    a partner going from an odd to an even count touches every submap of a robot whose poses alternate.  Nothing stale is reused
    silently: what these rules cannot see is the caller's to flag.

    With 'stacked_frame_descriptors' the similarity too follows the list: one roman_session_stacked_sim_list_dev
    writes the listed pairs' entries, the gate reads them there.  A call that lists every pair of every block (the first one),
    and a context without that entry, compute the whole blocks with roman_session_stacked_sim_dev as before.

    ValueError before any context is made: whatever submap_align_session refuses; a pool that shrank; a `touched` of the wrong
    length; a state made for other robot_pairs, another method, descriptor mode, gate, ground-truth pattern or num_solutions."""
    import torch
    from ..runtime import session_pair_list
    marks = [time.perf_counter()]
    sess = _session_setup(sm_params, pools, robot_pairs, sm_io, registration, gt_poses, num_solutions)
    p, R, blocks, gt_poses, keep, counts, aabb_mode = sess.p, sess.R, sess.blocks, sess.gt_poses, sess.keep, sess.counts, sess.aabb_mode
    # ---- what only a growing session can get wrong ----
    key = (tuple(blocks), type(sess.registration).__name__, getattr(sm_params, "method", None), sess.mode, aabb_mode, tuple(g is not None for g in gt_poses),
           num_solutions, int(sess.d))
    if state.key is not None and state.key != key:
        raise ValueError("the state was made by a call with other robot_pairs, another method, descriptor mode, gate, ground-truth pattern or "
                         "num_solutions: a SessionAlignState serves one kind of call")
    n_pool = [len(q.count) for q in p]
    if state.key is not None and any(n < m for n, m in zip(n_pool, state.n_pool)):
        raise ValueError("a pool shrank: between two calls pools may only grow by appending submaps")
    touched = [None] * R if touched is None else list(touched)
    if len(touched) != R or any(t is not None and np.asarray(t).reshape(-1).shape[0] != n for t, n in zip(touched, n_pool)):
        raise ValueError("touched must hold one entry per pool, each None or one flag per submap of that pool")

    views, vblocks, vcount, (sub_off, blk, pair_off, _) = _session_views(sess)      # (cut exactly as submap_align_session cuts them)

    # ---- the touched set: the caller's flags, what is new, and what differs from the bytes the state recorded ----
    def rows_of_view(v):
        """-> (uint8 (n, a) of what does not depend on the reads, uint8 (n, b) of what does) per non-empty submap of view v."""
        r, hs = views[v]
        n = int(counts[r])
        if hs is None:
            return np.zeros((n, 0), np.uint8), np.zeros((n, 0), np.uint8)
        as_bytes = lambda parts: np.concatenate([np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(n, -1)).view(np.uint8) for a in parts], axis=1)
        fixed = [hs["pos"], hs["time"]] + ([hs["pos_gt"]] if hs["pos_gt"] is not None else [])
        return as_bytes(fixed), as_bytes([hs["T_w"][0], hs["frames"][0], hs["frames"][1]] + ([hs["T_oc"]] if aabb_mode else []))
    seen = {(b, a): rows_of_view(vblocks[b][a]) for b in range(len(blocks)) for a in range(2)}
    flag = [np.zeros(n, dtype=bool) if t is None else np.asarray(t, dtype=bool).reshape(-1).copy() for t, n in zip(touched, n_pool)]
    first = state.key is None
    for r in range(R):
        if first:
            flag[r][:] = True
            continue
        flag[r][state.n_pool[r]:] = True
        flag[r][np.setdiff1d(keep[r], state.keep[r])] = True     # (it was empty)
    if not first:
        for (b, a), (fixed, posed) in seen.items():
            r = blocks[b][a]
            was_fixed, was_posed = state.seen[(b, a)]
            common, at_new, at_old = np.intersect1d(keep[r], state.keep[r], return_indices=True)
            if not len(common) or not fixed.shape[1] or not was_fixed.shape[1]:
                if len(common) and fixed.shape[1] != was_fixed.shape[1]:
                    flag[r][:] = True                            # (the block had no pair before, or has none now: nothing recorded to compare with)
                continue
            flag[r][common[(fixed[at_new] != was_fixed[at_old]).any(axis=1)]] = True
            flag[r][common[(posed[at_new] != was_posed[at_old]).any(axis=1)]] = True      # (it is read with another pose, in this block at least)
    local_flag = [flag[r][keep[r]] for r in range(R)]

    prm, Ms, result_of = _session_block_results(sess)
    nb = len(blocks)
    old = []                                                     # per block: the stored results re-indexed into Ms[b] -> (edges, hypotheses)
    for b, (r, s) in enumerate(blocks):
        if first:
            old.append((Ms[b].empty_edges(), None if num_solutions is None else {}))
        else:
            e, hy = _carry_over(Ms[b], state.results[blocks[b]], (state.keep[r], state.keep[s]), (keep[r], keep[s]))
            old.append(((e if e is not None else Ms[b].empty_edges()) if Ms[b].device_edges else None, hy))
    lst = session_pair_list(vcount, vblocks, [local_flag[r] for r, _ in views])
    total, L = int(pair_off[-1]), len(lst)
    cut = np.searchsorted(lst[:, 0], np.arange(nb + 1))          # block b's entries are lst[cut[b]:cut[b + 1]]

    def remember(out):
        state.key, state.n_pool, state.keep, state.seen, state.results, state.listed, state.total = key, n_pool, keep, seen, out, L, total
        marks.append(time.perf_counter())
        state.seconds = dict(zip(("host", "gate", "register"), np.diff(marks).tolist()))
        return out

    def merged(b, fresh_M=None, ti=None, tj=None, fresh_edges=None, fresh_hyps=None, timing=()):
        """Block b: the carried-over entries, and over them what this call computed for its listed pairs."""
        M, (edges, hyps) = Ms[b], old[b]
        li, lj = lst[cut[b]:cut[b + 1], 1].astype(np.int64), lst[cut[b]:cut[b + 1], 2].astype(np.int64)
        if fresh_M is not None:                                  # (a grid of one column: row k is the block's k-th listed pair)
            for name in _MATRICES:
                getattr(M, name)[li, lj] = getattr(fresh_M, name)[:, 0]
            for k, (i, j) in enumerate(zip(li.tolist(), lj.tolist())):
                M.associated_objs_mat[i][j] = fresh_M.associated_objs_mat[k][0]
        n1 = max(int(counts[blocks[b][1]]), 1)
        was_listed = np.zeros(int(counts[blocks[b][0]]) * n1 + 1, dtype=bool)
        was_listed[li * n1 + lj] = True
        if M.device_edges:
            kept = ~was_listed[edges["pairs"][:, 0] * n1 + edges["pairs"][:, 1]] if len(edges["pairs"]) else np.zeros(0, dtype=bool)
            parts = [dict(pairs=edges["pairs"][kept], t=edges["t"][kept], q=edges["q"][kept])] + ([fresh_edges] if fresh_edges is not None else [])
            pr = np.concatenate([np.asarray(e["pairs"], dtype=np.int64).reshape(-1, 2) for e in parts])
            order = np.lexsort((pr[:, 1], pr[:, 0]))             # loop order: row-major
            edges = dict(pairs=pr[order], t=np.concatenate([np.asarray(e["t"]).reshape(-1, 3) for e in parts])[order],
                         q=np.concatenate([np.asarray(e["q"]).reshape(-1, 4) for e in parts])[order])
        else:
            edges = None
        if hyps is not None:
            hyps = {k: v for k, v in hyps.items() if not was_listed[k[0] * n1 + k[1]]}
            hyps.update(fresh_hyps or {})
            hyps = dict(sorted(hyps.items()))
        return result_of(b, M, timing, edges, hyps)

    if L == 0:                                                   # nothing touched (or no pair at all): the stored results, re-indexed; no context is made
        return remember({blocks[b]: merged(b) for b in range(nb)})
    marks.append(time.perf_counter())
    ctx = _session_context(sess, "session_gate_list_dev")
    u = _session_uploads(torch, sess, views, sub_off, blk, pair_off)
    t, ptr = u.t, u.ptr
    t["list"] = u.up(lst)

    # ---- pass 1 of the listed pairs on the device: one enqueue, one synchronisation, one read-back.  With stacked descriptors the
    # similarity of the listed pairs (of the whole blocks where everything is listed), then the gate that reads it there ----
    one_pool = _session_pool(torch, sess, u.lv)
    g, gp, gate_kw = _session_pass1_front(torch, ctx, sess, u, sub_off, blk, pair_off, L, one_pool, sim_total=total, lst=lst)
    if aabb_mode:
        gate_kw["box_ptr"] = ptr(t["box"])
    ctx.session_gate_list_dev(gp, sub_off, blk, pair_off, lst, ptr(t["sub_off"]), ptr(t["blocks"]), ptr(t["pair_off"]), ptr(t["list"]), ptr(t["pos"]), ptr(t["T_w"]),
                              *[g[k].data_ptr() for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off")], **gate_kw)
    ctx.sync()
    todo_off = g["todo_off"].cpu().numpy().astype(np.int64)
    B = int(todo_off[-1])
    gpairs = g["pairs"][:B].cpu().numpy().astype(np.int64)
    h = {k: g[k].cpu().numpy() for k in ("dist", "flags", "yaw", "sim", "T_ij")}
    fresh, nearby, local, at = [], [], [], []                   # at[b]: the rows of fresh[b] that were registered
    for b, (r, s) in enumerate(blocks):                          # a block's listed entries as a grid of one column, then pass 1 as ever
        n1 = int(counts[s])
        lo, hi = int(cut[b]), int(cut[b + 1])
        lp_ = gpairs[todo_off[b]:todo_off[b + 1]] - np.array([sub_off[vblocks[b][0]], sub_off[vblocks[b][1]]], dtype=np.int64)
        if hi == lo:                                             # nothing of this block is listed: it is carried over as it is
            fresh.append(None); nearby.append(None); local.append(np.zeros((0, 2), dtype=np.int64)); at.append(np.zeros(0, dtype=np.int64))
            continue
        F = _GridResults(prm[b], sess.sm_io, hi - lo, 1)
        flags = h["flags"][lo:hi].reshape(-1, 1)
        near, todo = (flags & _abi.ROMAN_GRID_NEARBY) != 0, (flags & _abi.ROMAN_GRID_TODO) != 0
        F.pass1(h["dist"][lo:hi].reshape(-1, 1), near, (flags & _abi.ROMAN_GRID_SKIP) != 0, (flags & _abi.ROMAN_GRID_GATED) != 0,
                h["yaw"][lo:hi].reshape(-1, 1), h["sim"][lo:hi].reshape(-1, 1), h["T_ij"][lo:hi].reshape(-1, 1, 4, 4))
        k = np.nonzero(todo[:, 0])[0]                            # the listed entries that are TODO: the block's compact slots, in this order
        if not np.array_equal(lp_, lst[lo:hi, 1:][k].astype(np.int64)):
            raise _abi.RomanHipError(f"roman_session_gate_list_dev: the compact pair list of block {blocks[b]} is not its listed TODO pairs in list order")
        fresh.append(F); nearby.append(near); local.append(lp_); at.append(k)
    marks.append(time.perf_counter())
    if B == 0:
        return remember({blocks[b]: merged(b, fresh[b]) for b in range(nb)})

    # ---- ONE batch over the ONE pool, as in submap_align_session; a block's records into its one-column grid ----
    parts, per_pair = _session_register(torch, ctx, sess, u, gpairs, todo_off, one_pool, g)
    out = {}
    for b, part in enumerate(parts):
        n = len(at[b])
        edges = Ms[b].empty_edges()
        if n:
            edges = _records_into_results(fresh[b], part, at[b], np.zeros(n, dtype=np.int64), nearby[b])
            if edges is not None:                                # (row of the one-column grid -> the pair it stands for)
                edges["pairs"] = lst[int(cut[b]):int(cut[b + 1]), 1:][edges["pairs"][:, 0]].astype(np.int64).reshape(-1, 2)
        out[blocks[b]] = merged(b, fresh[b], fresh_edges=edges, fresh_hyps=_hypotheses_of(part, local[b][:, 0], local[b][:, 1]), timing=[per_pair] * n)
    return remember(out)


# ---------------------------------------------------------------------------------------------
# writers (row f3): the wire formats g2o_file_fusion / Kimera-RPGO consume
# ---------------------------------------------------------------------------------------------
def nearest_index(times, t):
    """Index of the trajectory sample closest to time t (what robotdatapy's PoseData.idx(t, force_single=True) returns)."""
    times = np.asarray(times, dtype=np.float64)
    return int(np.argmin(np.abs(times - t)))


def loop_closure_edges(results: SubmapAlignResults, submaps):
    """The (i, j, T_pi_pj) triples the reference writes ([REF roman/align/results.py:156-171]): pairs with at
    least `lc_association_thresh` associations (and far enough apart in time for single-robot runs), with the
    estimated submap-centre transform composed into pose-frame i -> pose-frame j."""
    if getattr(results, "lc_edges", None) is not None:
        return [(i, j, T) for (i, j, T, _, _) in _device_edges(results, submaps)]
    out = []
    p, io = results.submap_align_params, results.submap_io
    for i in range(len(submaps[0])):
        for j in range(len(submaps[1])):
            if not (results.clipper_num_associations[i, j] >= io.lc_association_thresh):
                continue
            if np.abs(submaps[0][i].time - submaps[1][j].time) < p.single_robot_lc_time_thresh and p.single_robot_lc:
                continue
            T_ci_cj = results.T_ij_hat_mat[i, j]
            T_odomi_ci = submaps[0][i].pose_gravity_aligned
            T_odomj_cj = submaps[1][j].pose_gravity_aligned
            T_odomi_pi = submaps[0][i].pose_flu
            T_odomj_pj = submaps[1][j].pose_flu
            T_pi_pj = np.linalg.inv(T_odomi_pi) @ T_odomi_ci @ T_ci_cj @ np.linalg.inv(T_odomj_cj) @ T_odomj_pj
            out.append((i, j, T_pi_pj))
    return out


def _device_edges(results, submaps):
    """(i, j, T_pi_pj, t, q) per accepted pair from the edges the device computed (submap_align_grid): no per-pair matrix
    work.  Leaves the submaps as the per-pair loop does: it reads `pose_gravity_aligned` of both submaps of every accepted
    pair, which may flatten `pose_flu` in place."""
    e = results.lc_edges
    pairs, t, q = np.asarray(e["pairs"]).reshape(-1, 2), np.asarray(e["t"]).reshape(-1, 3), np.asarray(e["q"]).reshape(-1, 4)
    for r in range(2):
        ks, counts = np.unique(pairs[:, r], return_counts=True)
        for k, n in zip(ks.tolist(), counts.tolist()):
            _read_times(submaps[r][k], "pose_gravity_aligned", "pose_flu", n)      # (stops at the fixed point a yaw-only pose is)
    T = np.tile(np.eye(4), (pairs.shape[0], 1, 1))
    T[:, :3, :3] = _quat_to_matrix(q); T[:, :3, 3] = t
    return [(int(pairs[k, 0]), int(pairs[k, 1]), T[k], t[k].copy(), q[k].copy()) for k in range(pairs.shape[0])]


def _edges_xyz_quat(results, submaps):
    """(i, j, translation, quaternion xyzw) of every loop closure: from the device's edges when the result carries them,
    otherwise loop_closure_edges() + transform_to_xyz_quat()."""
    if getattr(results, "lc_edges", None) is not None:
        return [(i, j, t, q) for (i, j, _, t, q) in _device_edges(results, submaps)]
    return [(i, j) + transform_to_xyz_quat(T) for (i, j, T) in loop_closure_edges(results, submaps)]


def write_g2o(path, results: SubmapAlignResults, submaps, trajectory_times):
    """`.g2o` loop closures, same text as [REF roman/align/results.py:156-194]: per edge a `# LC: <n>` comment
    (read by g2o_file_fusion, [REF roman/offline_rpgo/g2o_file_fusion.py:54-68]) and an `EDGE_SE3:QUAT` line with
    the upper triangle of the information matrix.  trajectory_times[r]: pose timestamps of robot r's odometry."""
    io = results.submap_io
    I_t, I_r = 1 / (io.g2o_t_std ** 2), 1 / (io.g2o_r_std ** 2)
    I = np.diag([I_t, I_t, I_t, I_r, I_r, I_r])
    with open(path, 'w') as f:
        for (i, j, t, q) in _edges_xyz_quat(results, submaps):
            idx_a = nearest_index(trajectory_times[0], submaps[0][i].time)
            idx_b = nearest_index(trajectory_times[1], submaps[1][j].time)
            f.write(f"# LC: {int(results.clipper_num_associations[i, j])}\n")
            f.write(f"EDGE_SE3:QUAT a{idx_a} b{idx_b} \t")
            f.write(f"{t[0]} {t[1]} {t[2]} \t")
            f.write(f"{q[0]} {q[1]} {q[2]} {q[3]} \t")
            for ii in range(6):
                for jj in range(6):
                    if jj < ii:
                        continue
                    f.write(f"{I[ii, jj]} ")
                f.write("\t")
            f.write("\n")


def write_lc_json(path, results: SubmapAlignResults, submaps):
    """Loop-closure json, same records as [REF roman/align/results.py:172-179,196-198]."""
    out = []
    for (i, j, t, q) in _edges_xyz_quat(results, submaps):
        out.append({
            'seconds': [int(submaps[0][i].time), int(submaps[1][j].time)],
            'nanoseconds': [int((submaps[0][i].time % 1) * 1e9), int((submaps[1][j].time % 1) * 1e9)],
            'names': results.submap_io.robot_names,
            'translation': t.tolist(),
            'rotation': q.tolist(),
            'rotation_convention': 'xyzw',
        })
    with open(path, 'w') as f:
        json.dump(out, f, indent=4)


def write_matrix_pickle(path, results: SubmapAlignResults):
    """[REF roman/align/results.py:128-132]: the five result matrices as one pickled list."""
    with open(path, 'wb') as f:
        pickle.dump([results.robots_nearby_mat, results.clipper_angle_mat, results.clipper_dist_mat,
                     results.clipper_num_associations, results.submap_yaw_diff_mat], f)


def write_timing(path, results: SubmapAlignResults, submaps):
    """[REF roman/align/results.py:139-144]"""
    with open(path, 'w') as f:
        f.write(f"Total number of submaps: {len(submaps[0])} x {len(submaps[1])} = {len(submaps[0])*len(submaps[1])}\n")
        f.write(f"Average time per registration: {np.mean(results.timing_list):.4f} seconds\n")
        f.write(f"Total time: {np.sum(results.timing_list):.4f} seconds\n")
        f.write(f"Total number of objects: {np.sum([len(submap) for submap in submaps[0] + submaps[1]])}\n")
        f.write(f"Average number of obects per map: {np.mean([len(submap) for submap in submaps[0] + submaps[1]]):.2f}\n")


def write_submaps_json(path, robot_name, map_segments, robot_submaps):
    """Per-robot `<name>.sm.json` ([REF roman/align/results.py:200-243]): one record per map segment that carries
    a point cloud (segments without one are skipped, as the reference's bare `except: continue` does) and one
    per submap with its gravity-aligned pose."""
    sm_json = {'segments': [], 'submaps': []}
    secs_nsecs = lambda t: {'seconds': int(t), 'nanoseconds': int((t - int(t)) * 1e9)}
    for segment in map_segments:
        try:
            sm_json['segments'].append({
                'robot_name': robot_name,
                'segment_index': segment.id,
                'centroid_odom': np.mean(segment.points, axis=0).tolist(),
                'shape_attributes': {'volume': segment.volume, 'linearity': segment.linearity,
                                     'planarity': segment.planarity, 'scattering': segment.scattering},
                'first_seen': secs_nsecs(segment.first_seen),
                'last_seen': secs_nsecs(segment.last_seen)})
        except Exception:
            continue
    for j, sm in enumerate(robot_submaps):
        x = np.concatenate(transform_to_xyz_quat(sm.pose_gravity_aligned))
        sm_json['submaps'].append({
            'submap_index': j,
            'T_odom_submap': {'tx': x[0], 'ty': x[1], 'tz': x[2], 'qx': x[3], 'qy': x[4], 'qz': x[5], 'qw': x[6]},
            'robot_name': robot_name,
            'seconds': int(sm.time),
            'nanoseconds': int((sm.time % 1) * 1e9),
            'segment_indices': [segment.id for segment in sm.segments]})
    with open(path, 'w') as f:
        json.dump(sm_json, f, indent=4)
