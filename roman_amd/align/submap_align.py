"""Submap-pair loop and result writers on the batched HIP path.

Mirrors the part of the reference's caller that surrounds the hot path:

  * `submap_align()` [REF roman/align/submap_align.py:74-220] — gating (distance / AABB, submap descriptor
    similarity, `skip_distance`, shared-segment removal for single-robot loop closures), `register()` +
    `T_align()` for every surviving pair, the gravity post-filters, the error metrics against the reference
    transform, and the result matrices.  Instead of the serial double loop with a device round trip per pair,
    all surviving pairs go to ONE `roman_align_batch` call and every submap is packed once.
    `submap_align_grid()` vectorises pass 1 over the grid and leaves pass 2 and the edges to the device; `submap_align_pools()`
    starts from two device-resident submap pools (align.submaps.SubmapPool) and runs pass 1 on the device too
    (roman_grid_gate_dev).
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
from typing import Callable, List, Optional, Sequence

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from .. import _abi
from ..runtime import LcInputs
from .batch import AlignmentBatch, pack_submaps, run_batch, run_lc_batch, run_lc_batch_ids
from .dist_reg_with_pruning import _zyx_euler
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
            if np.isclose(norm_prod, 0.0, atol=1e-9, rtol=0.0):
                return 0.0
            return np.dot(desc1, desc2) / norm_prod
        d1 = desc1.reshape(desc1.shape[0], 1, desc1.shape[1]); d2 = desc2.reshape(1, desc2.shape[0], desc2.shape[1])
        norm_prods = np.linalg.norm(d1, axis=2) * np.linalg.norm(d2, axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            sims = np.sum(d1 * d2, axis=2) / norm_prods
        sims[np.isclose(norm_prods, 0.0, atol=1e-9, rtol=0.0)] = 0.0
        return np.max(sims)


def stacked_similarity(ctx, descs0, descs1):
    """Best pairwise cosine between the frame descriptors of every submap of robot 0 and every submap of robot 1
    ([REF roman/map/map.py:152-162]) -> (S0, S1).  One cosine kernel over all frames, then a segmented maximum."""
    o0 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs0])]).astype(np.int64)
    o1 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs1])]).astype(np.int64)
    frames = ctx.cosine_matrix(np.concatenate(descs0, axis=0), np.concatenate(descs1, axis=0))     # zero-norm frames: 0
    return np.maximum.reduceat(np.maximum.reduceat(frames, o0[:-1], axis=0), o1[:-1], axis=1)


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
    # submap_align_grid only: the loop-closure edges as the device computed them — {'pairs': (K, 2) int (i, j) in loop order,
    # 't': (K, 3), 'q': (K, 4) xyzw}.  loop_closure_edges() and the writers then do no per-pair matrix work.
    lc_edges: Optional[dict] = None


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
    nan = lambda *s: np.zeros(s) * np.nan
    clipper_angle_mat, clipper_dist_mat, clipper_num_associations = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    similarity_mat, robots_nearby_mat, submap_yaw_diff_mat = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    T_ij_mat, T_ij_hat_mat = nan(n0, n1, 4, 4), nan(n0, n1, 4, 4)
    associated_objs_mat = [[[] for _ in range(n1)] for _ in range(n0)]
    total_time_t0 = time.time()

    # ---- submap-descriptor gate (row f2): every cosine of the S0 x S1 gate in ONE device call (k_cos, f64 matrix
    # core).  Plain vector descriptors: the S0 x S1 cosine matrix itself.  Stacked per-frame descriptors
    # ([REF roman/map/map.py:152-162]: the best cosine over all frame pairs, zero-norm frames scoring 0): all frames
    # of all submaps go through the same kernel at once and the per-pair maximum is a segmented reduction of its
    # output.  (The CPU test double uses the per-pair numpy form below.) -----------------------------------------
    sim_all = None
    if sm_params.submap_descriptor is not None and compute is run_batch and n0 and n1:
        descs = [[np.asarray(sm.descriptor) for sm in submaps[r]] for r in range(2)]
        flat = [d for r in range(2) for d in descs[r]]
        if all(d.ndim == 1 for d in flat):
            sim_all = registration._context().cosine_matrix(np.stack(descs[0]), np.stack(descs[1]))
        elif all(d.ndim == 2 and d.shape[0] > 0 and d.shape[1] == flat[0].shape[1] for d in flat):
            sim_all = stacked_similarity(registration._context(), descs[0], descs[1])

    # ---- pass 1: gating, reference transforms, the list of pairs to register ([REF :93-149]) -------------------
    todo = []                                            # (i, j, segs_i, segs_j)
    skipped_sim = []
    for i in range(n0):
        for j in range(n1):
            si, sj = submaps[0][i], submaps[1][j]
            if si.has_gt and sj.has_gt:
                submap_distance = np.linalg.norm(si.position_gt - sj.position_gt)
            else:
                submap_distance = np.linalg.norm(si.position - sj.position)
            if (not sm_params.force_fill_submaps and sm_params.submap_radius is not None and submap_distance < sm_params.submap_radius * 2) or \
                    ((sm_params.force_fill_submaps or sm_params.submap_radius is None) and len(si) and len(sj)
                     and aabb_intersects(si.segments_as_global_points, sj.segments_as_global_points)):
                robots_nearby_mat[i, j] = submap_distance
            segs_i, segs_j = list(si.segments), list(sj.segments)
            if sm_params.single_robot_lc:                # self loop closures: drop the segments both submaps hold
                common = {seg.id for seg in segs_i} & {seg.id for seg in segs_j}
                segs_i = [s for s in segs_i if s.id not in common]; segs_j = [s for s in segs_j if s.id not in common]
            T_wi = si.pose_gravity_aligned_gt if sm_io.gt_available[0] else si.pose_gravity_aligned
            T_wj = sj.pose_gravity_aligned_gt if sm_io.gt_available[1] else sj.pose_gravity_aligned
            T_ij = np.linalg.inv(T_wi) @ T_wj
            if not np.isnan(robots_nearby_mat[i, j]):
                submap_yaw_diff_mat[i, j] = np.abs(np.rad2deg(transform_to_xyzrpy(T_ij)[5]))
            submap_sim = np.inf if sm_params.submap_descriptor is None else (sim_all[i, j] if sim_all is not None else Submap.similarity(si, sj))
            T_ij_mat[i, j] = T_ij
            if submap_distance > sm_io.skip_distance:
                clipper_num_associations[i, j] = 0
                T_ij_hat_mat[i, j] = nan(4, 4)
                continue
            similarity_mat[i, j] = submap_sim
            if submap_sim < sm_params.submap_descriptor_thresh:
                skipped_sim.append((i, j, len(segs_i), len(segs_j)))
            else:
                todo.append((i, j, segs_i, segs_j))

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
        lists = [registration._association_list(a, b) if (len(a) and len(b)) else None for (_, _, a, b) in todo]
        if any(l is not None for l in lists):            # pruning plugins score explicit association lists
            from ..clipperpy.utils import create_all_to_all
            lists = [l if l is not None else create_all_to_all(len(a), len(b)) for l, (_, _, a, b) in zip(lists, todo)]
            batch.assoc_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
            batch.assoc = np.concatenate(lists, axis=0).astype(np.int32)
        t0 = time.time()
        res = compute(registration, batch)
        timing_list = [(time.time() - t0) / len(todo)] * len(todo)

    # ---- pass 2: post-filters, error metrics, result matrices ([REF :160-200]) ---------------------------------
    def report(i, j, T_ij_hat, theta, dist, associations, len_i, len_j):
        if not np.isnan(robots_nearby_mat[i, j]):
            clipper_angle_mat[i, j] = np.abs(np.rad2deg(theta)); clipper_dist_mat[i, j] = dist
        clipper_num_associations[i, j] = len(associations)
        T_ij_hat_mat[i, j] = T_ij_hat
        associated_objs_mat[i][j] = associations

    prune_tilt = registration.roll_pitch_thresh if getattr(registration, "use_gravity", False) else None
    for (i, j, li, lj) in skipped_sim:
        report(i, j, nan(4, 4), 180.0, 1e6, [], li, lj)
    for b, (i, j, segs_i, segs_j) in enumerate(todo):
        T_ij = T_ij_mat[i, j]
        failed = bool(res.status[b] & (_abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_EMPTY_MAP))   # T_align would raise
        associations = res.assoc[b]
        if not failed:
            T_ij_hat = np.array(res.T[b], dtype=np.float64)
            if prune_tilt is not None:                   # DistRegWithPruning.register's own check [REF dist_reg_with_pruning.py:38-45]
                _, pitch, roll = _zyx_euler(T_ij_hat[:sm_params.dim, :sm_params.dim])
                failed = not (np.abs(roll) < prune_tilt and np.abs(pitch) < prune_tilt)
        if not failed:
            if sm_params.dim == 2:
                # The reference multiplies a 3x3 estimate into the 4x4 reference transform here and cannot run
                # ([REF :159-162]); the planar estimate is lifted to SE(3) (identity in z) instead.
                T2 = T_ij_hat; T_ij_hat = np.eye(4); T_ij_hat[:2, :2] = T2[:2, :2]; T_ij_hat[:2, 3] = T2[:2, 2]
                T_error = np.linalg.inv(T_ij_hat) @ T_ij
                theta = np.arctan2(T_error[1, 0], T_error[0, 0]); dist = np.linalg.norm(T_error[:2, 3])
            else:
                if sm_params.force_rm_upside_down:       # GravityConstraintError branch [REF :167-170]
                    xyzrpy = transform_to_xyzrpy(T_ij_hat)
                    failed = bool(np.abs(xyzrpy[3]) > np.deg2rad(90.) or np.abs(xyzrpy[4]) > np.deg2rad(90.))
                if not failed:
                    if sm_params.force_rm_lc_roll_pitch:
                        T_ij_hat = transform_rm_roll_pitch(T_ij_hat)
                    T_error = np.linalg.inv(T_ij_hat) @ T_ij
                    theta = Rot.from_matrix(T_error[:3, :3]).magnitude(); dist = np.linalg.norm(T_error[:3, 3])
        if failed:                                       # the except-branch sentinel [REF :179-184]
            T_ij_hat, theta, dist, associations = nan(4, 4), 180.0, 1e6, []
        report(i, j, T_ij_hat, theta, dist, associations, len(segs_i), len(segs_j))

    return SubmapAlignResults(
        robots_nearby_mat=robots_nearby_mat, clipper_angle_mat=clipper_angle_mat, clipper_dist_mat=clipper_dist_mat,
        clipper_num_associations=clipper_num_associations,
        similarity_mat=similarity_mat if sm_params.submap_descriptor is not None else None,
        submap_yaw_diff_mat=submap_yaw_diff_mat, T_ij_mat=T_ij_mat, T_ij_hat_mat=T_ij_hat_mat,
        associated_objs_mat=associated_objs_mat, timing_list=timing_list, submap_align_params=sm_params,
        submap_io=sm_io, total_time=time.time() - total_time_t0)


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


def _host_similarity(descs0, descs1):
    """Submap.similarity for every pair at once (the CPU double's descriptor gate): vector descriptors or stacked frames."""
    flat = descs0 + descs1
    if all(d.ndim == 1 for d in flat):
        A, B = np.stack(descs0), np.stack(descs1)
        norm_prod = np.linalg.norm(A, axis=1)[:, None] * np.linalg.norm(B, axis=1)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            sim = (A @ B.T) / norm_prod
        sim[np.isclose(norm_prod, 0.0, atol=1e-9, rtol=0.0)] = 0.0
        return sim
    if all(d.ndim == 2 and d.shape[0] > 0 and d.shape[1] == flat[0].shape[1] for d in flat):
        o0 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs0])]).astype(np.int64)
        o1 = np.concatenate([[0], np.cumsum([d.shape[0] for d in descs1])]).astype(np.int64)
        A, B = np.concatenate(descs0, axis=0), np.concatenate(descs1, axis=0)
        norm_prod = np.linalg.norm(A, axis=1)[:, None] * np.linalg.norm(B, axis=1)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            frames = (A @ B.T) / norm_prod
        frames[np.isclose(norm_prod, 0.0, atol=1e-9, rtol=0.0)] = 0.0
        return np.maximum.reduceat(np.maximum.reduceat(frames, o0[:-1], axis=0), o1[:-1], axis=1)
    return None


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


def _records_into_results(res, ti, tj, nearby, device_edges, clipper_angle_mat, clipper_dist_mat, clipper_num_associations,
                          T_ij_hat_mat, associated_objs_mat):
    """Pass 2 of the grid forms ([REF roman/align/submap_align.py:186-200]): the tail's records of the registered pairs (ti, tj)
    into the result matrices, IN PLACE -> the loop-closure edges (None unless the device decided them)."""
    rec = res.records
    if np.any(rec["flags"] & (_abi.ROMAN_LC_SKIPPED | _abi.ROMAN_LC_INTERNAL)):
        raise _abi.RomanHipError("the batched call left problems without a result (ROMAN_LC_SKIPPED / ROMAN_LC_INTERNAL records)")
    near = nearby[ti, tj]
    clipper_angle_mat[ti[near], tj[near]] = np.abs(np.rad2deg(rec["theta"][near]))
    clipper_dist_mat[ti[near], tj[near]] = rec["dist"][near]
    clipper_num_associations[ti, tj] = rec["n_assoc"]
    T_ij_hat_mat[ti, tj] = rec["T_hat"]
    failed = (rec["flags"] & _abi.ROMAN_LC_FAILED) != 0
    for b in np.nonzero(~failed)[0].tolist():            # (placing the association arrays: no arithmetic)
        associated_objs_mat[ti[b]][tj[b]] = res.assoc[b]
    if not device_edges:
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
    an id is not an integer that int64 holds.

    `compute(registration, AlignmentBatch, runtime.LcInputs) -> runtime.LoopClosureResult` defaults to the HIP path
    (`run_lc_batch`); tests inject a CPU double."""
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    if isinstance(registration, RansacReg):
        raise NotImplementedError("submap_align_grid builds on roman_align_lc_batch; RANSAC registration has no device tail yet "
                                  "(use submap_align)")
    on_device = compute is None
    compute = compute or run_lc_batch
    S = [list(submaps[0]), list(submaps[1])]
    n0, n1 = len(S[0]), len(S[1])
    nan = lambda *s: np.zeros(s) * np.nan
    clipper_angle_mat, clipper_dist_mat, clipper_num_associations = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    similarity_mat, robots_nearby_mat, submap_yaw_diff_mat = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    T_ij_mat, T_ij_hat_mat = nan(n0, n1, 4, 4), nan(n0, n1, 4, 4)
    associated_objs_mat = [[[] for _ in range(n1)] for _ in range(n0)]
    total_time_t0 = time.time()
    make = lambda lc_edges=None, timing_list=(): SubmapAlignResults(
        robots_nearby_mat=robots_nearby_mat, clipper_angle_mat=clipper_angle_mat, clipper_dist_mat=clipper_dist_mat,
        clipper_num_associations=clipper_num_associations,
        similarity_mat=similarity_mat if sm_params.submap_descriptor is not None else None,
        submap_yaw_diff_mat=submap_yaw_diff_mat, T_ij_mat=T_ij_mat, T_ij_hat_mat=T_ij_hat_mat,
        associated_objs_mat=associated_objs_mat, timing_list=list(timing_list), submap_align_params=sm_params,
        submap_io=sm_io, total_time=time.time() - total_time_t0, lc_edges=lc_edges)
    device_edges = sm_io.lc_association_thresh > 0       # (a threshold <= 0 would accept pairs that never reach the device)
    empty_edges = dict(pairs=np.zeros((0, 2), np.int64), t=np.zeros((0, 3)), q=np.zeros((0, 4))) if device_edges else None
    if n0 == 0 or n1 == 0:
        return make(empty_edges)

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
    robots_nearby_mat[nearby] = dist[nearby]
    T_ij_mat[:] = np.matmul(np.linalg.inv(T_w[0])[:, None, :, :], T_w[1][None, :, :, :])
    yaw = np.arctan2(T_ij_mat[:, :, 1, 0], T_ij_mat[:, :, 0, 0])      # the fixed-axis xyz yaw of a rotation about z
    submap_yaw_diff_mat[nearby] = np.abs(np.rad2deg(yaw[nearby]))
    if sm_params.submap_descriptor is None:
        sim = np.full((n0, n1), np.inf)
    else:
        descs = [[np.asarray(sm.descriptor) for sm in S[r]] for r in range(2)]
        flat = descs[0] + descs[1]
        sim = None
        if on_device:                                    # row f2: every cosine of the gate in ONE device call
            if all(d.ndim == 1 for d in flat):
                sim = registration._context().cosine_matrix(np.stack(descs[0]), np.stack(descs[1]))
            elif all(d.ndim == 2 and d.shape[0] > 0 and d.shape[1] == flat[0].shape[1] for d in flat):
                sim = stacked_similarity(registration._context(), descs[0], descs[1])
        else:
            sim = _host_similarity(descs[0], descs[1])
        if sim is None:                                  # mixed descriptor kinds: the per-pair definition
            sim = np.array([[Submap.similarity(si, sj) for sj in S[1]] for si in S[0]], dtype=np.float64)
    skip = dist > sm_io.skip_distance
    clipper_num_associations[skip] = 0
    similarity_mat[~skip] = sim[~skip]
    with np.errstate(invalid="ignore"):
        gated = ~skip & (sim < sm_params.submap_descriptor_thresh)
    todo = ~skip & ~gated
    # pairs the descriptor gate stopped: the sentinels of [REF :179-184]
    clipper_num_associations[gated] = 0
    clipper_angle_mat[gated & nearby] = np.abs(np.rad2deg(180.0)); clipper_dist_mat[gated & nearby] = 1e6
    ti, tj = np.nonzero(todo)                            # row-major: the order of the pair loop
    B = int(ti.shape[0])
    if B == 0:
        return make(empty_edges)

    # ---- the hot path: every submap (variant) packed once, ONE batched call with the tail behind it ---------
    scorer = getattr(type(registration), "_associations_to_score", None)
    host_lists = scorer is not None and scorer is not ObjectRegistration._associations_to_score
    ui, uj = np.unique(ti), np.unique(tj)
    pool = [list(S[0][i].segments) for i in ui] + [list(S[1][j].segments) for j in uj]
    pool_ids = None
    if sm_params.single_robot_lc and on_device and not host_lists:
        pool_ids = _int64_ids(pool)                      # self loop closures: the device drops the segments both submaps hold
    if not sm_params.single_robot_lc or pool_ids is not None:
        slot_i = np.zeros(n0, dtype=np.int64); slot_i[ui] = np.arange(len(ui))
        slot_j = np.zeros(n1, dtype=np.int64); slot_j[uj] = len(ui) + np.arange(len(uj))
        ii, jj = slot_i[ti], slot_j[tj]
        pair_segs = None
    else:                                                # ... or the host does, per pair: a reduced copy of both submaps for every pair
        pool, pair_segs = [], []
        for i, j in zip(ti.tolist(), tj.tolist()):
            segs_i, segs_j = list(S[0][i].segments), list(S[1][j].segments)
            common = {seg.id for seg in segs_i} & {seg.id for seg in segs_j}
            segs_i = [s for s in segs_i if s.id not in common]; segs_j = [s for s in segs_j if s.id not in common]
            pool.append(segs_i); pool.append(segs_j); pair_segs.append((segs_i, segs_j))
        ii, jj = 2 * np.arange(B), 2 * np.arange(B) + 1
    feats, offs = pack_submaps(registration, pool)
    plen = np.diff(offs).astype(np.int32)
    batch = AlignmentBatch(feats, offs[ii].astype(np.int64), plen[ii], offs[jj].astype(np.int64), plen[jj],
                           pair_index=np.stack([ti, tj], axis=1), ids=pool_ids)
    if host_lists:
        # a pruning plugin scores explicit association lists: its host prefilter reads both maps of a pair
        segs_of = (lambda b: (pool[ii[b]], pool[jj[b]])) if pair_segs is None else (lambda b: pair_segs[b])
        lists = [registration._association_list(*segs_of(b)) if (plen[ii[b]] and plen[jj[b]]) else None for b in range(B)]
        if any(l is not None for l in lists):
            from ..clipperpy.utils import create_all_to_all
            lists = [l if l is not None else create_all_to_all(int(plen[ii[b]]), int(plen[jj[b]])) for b, l in enumerate(lists)]
            batch.assoc_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
            batch.assoc = np.concatenate(lists, axis=0).astype(np.int32)
    frames = [{int(k): _edge_frames(S[r][int(k)]) for k in np.unique(t)} for r, t in ((0, ti), (1, tj))]
    FL = np.tile(np.eye(4), (n0, 1, 1)); FR = np.tile(np.eye(4), (n1, 1, 1))
    for k, f in frames[0].items():
        FL[k] = f[0]
    for k, f in frames[1].items():
        FR[k] = f[1]
    times = [np.array([float(sm.time) for sm in S[r]]) for r in range(2)]
    enable = np.ones(B, dtype=np.int32)
    if sm_params.single_robot_lc:                        # the time gate of [REF roman/align/results.py:160-162]
        enable[np.abs(times[0][ti] - times[1][tj]) < sm_params.single_robot_lc_time_thresh] = 0
    lc = LcInputs(dim=sm_params.dim, force_rm_upside_down=sm_params.force_rm_upside_down,
                  force_rm_lc_roll_pitch=sm_params.force_rm_lc_roll_pitch,
                  tilt_thresh=registration.roll_pitch_thresh if getattr(registration, "use_gravity", False) else None,
                  lc_association_thresh=int(np.ceil(sm_io.lc_association_thresh)) if device_edges else 1,
                  T_ref=T_ij_mat[ti, tj], enable=enable, FL=FL, iL=ti, FR=FR, iR=tj)
    t0 = time.time()
    res = run_lc_batch_ids(registration, batch, lc) if pool_ids is not None else compute(registration, batch, lc)
    timing_list = [(time.time() - t0) / B] * B

    # ---- pass 2: the records into the result matrices -------------------------------------------------------
    lc_edges = _records_into_results(res, ti, tj, nearby, device_edges, clipper_angle_mat, clipper_dist_mat, clipper_num_associations,
                                     T_ij_hat_mat, associated_objs_mat)
    return make(lc_edges, timing_list)


def submap_align_pools(sm_params, pools, sm_io: Optional[SubmapAlignIO] = None, registration=None, gt_poses=(None, None)) -> SubmapAlignResults:
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

    Not covered — ValueError; SubmapPool.to_submaps() + submap_align_grid is the way: single_robot_lc over submaps that share
    segment ids (one pool against itself), force_fill_submaps / no submap_radius (the AABB gate), stacked or frame descriptors,
    RansacReg, registration plugins with a host prefilter."""
    import torch
    from ..runtime import LoopClosureResult, grid_gate_params, lc_record_dtype, stats_dtype
    from .pipeline import issue_chunked
    sm_io = sm_io or SubmapAlignIO()
    registration = registration or sm_params.get_object_registration()
    way = " (not on the device-resident path: use SubmapPool.to_submaps() + submap_align_grid)"
    p = list(pools)
    if len(p) != 2:
        raise ValueError("pools must hold two SubmapPool objects")
    if isinstance(registration, RansacReg):
        raise ValueError("RansacReg has no device tail" + way)
    if sm_params.force_fill_submaps or sm_params.submap_radius is None:
        raise ValueError("force_fill_submaps / submap_radius None gate pairs on bounding boxes" + way)
    if sm_params.submap_descriptor not in (None, 'mean_semantic'):
        raise ValueError(f"submap_descriptor {sm_params.submap_descriptor!r}: stacked or frame descriptors are not in the pool" + way)
    scorer = getattr(type(registration), "_associations_to_score", None)
    if scorer is not None and scorer is not ObjectRegistration._associations_to_score:
        raise ValueError("the registration plugin prefilters association lists on the host" + way)
    if sm_params.single_robot_lc:
        shared = p[0] is p[1] or np.intersect1d(p[0].ids[p[0].src >= 0], p[1].ids[p[1].src >= 0]).size > 0
        if shared:
            raise ValueError("single_robot_lc over submaps that share segment ids: the shared-segment removal has no device-pointer form yet" + way)
    d = 0
    if sm_params.submap_descriptor is not None:
        if p[0].desc_dev is None or p[1].desc_dev is None:
            raise ValueError("submap_descriptor 'mean_semantic' needs pools built with it (build_submap_pool keeps the descriptors on the device)")
        d = int(p[0].desc_dev.shape[1])
        if int(p[1].desc_dev.shape[1]) != d:
            raise ValueError("the two pools have descriptors of different lengths")
    for r in range(2):
        if sm_io.gt_available[r] and gt_poses[r] is None:
            raise ValueError(f"sm_io.gt_available[{r}] is set without gt_poses[{r}]")
    ctx = registration._context()
    dev = p[0].pool.device
    on_host = dev.type == "cpu"                              # CPU tensors + a stand-in context (tests)
    wait_torch = (lambda: None) if on_host else (lambda: torch.cuda.current_stream(dev).synchronize())
    keep = [q.nonempty for q in p]                           # [REF roman/map/map.py:341]: the reference drops the empty submaps
    n0, n1 = len(keep[0]), len(keep[1])
    nan = lambda *s: np.zeros(s) * np.nan
    clipper_angle_mat, clipper_dist_mat, clipper_num_associations = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    similarity_mat, robots_nearby_mat, submap_yaw_diff_mat = nan(n0, n1), nan(n0, n1), nan(n0, n1)
    T_ij_mat, T_ij_hat_mat = nan(n0, n1, 4, 4), nan(n0, n1, 4, 4)
    associated_objs_mat = [[[] for _ in range(n1)] for _ in range(n0)]
    total_time_t0 = time.time()
    make = lambda lc_edges=None, timing_list=(): SubmapAlignResults(
        robots_nearby_mat=robots_nearby_mat, clipper_angle_mat=clipper_angle_mat, clipper_dist_mat=clipper_dist_mat,
        clipper_num_associations=clipper_num_associations,
        similarity_mat=similarity_mat if sm_params.submap_descriptor is not None else None,
        submap_yaw_diff_mat=submap_yaw_diff_mat, T_ij_mat=T_ij_mat, T_ij_hat_mat=T_ij_hat_mat,
        associated_objs_mat=associated_objs_mat, timing_list=list(timing_list), submap_align_params=sm_params,
        submap_io=sm_io, total_time=time.time() - total_time_t0, lc_edges=lc_edges)
    device_edges = sm_io.lc_association_thresh > 0
    empty_edges = dict(pairs=np.zeros((0, 2), np.int64), t=np.zeros((0, 3)), q=np.zeros((0, 4))) if device_edges else None
    if n0 == 0 or n1 == 0:
        return make(empty_edges)

    # ---- per submap, on the host (O(S)): centre, the pose the reference transform is built from, time, the edge frames —
    # through the stand-in Submap's own properties, read as often as the pair loop reads them (submap_align_grid does the same) ----
    other = (n1, n0)
    pos, pos_gt, T_w, times, frames = [], [], [], [], []
    for r in range(2):
        c = p[r].centers
        gt = None if gt_poses[r] is None else np.asarray(gt_poses[r], dtype=np.float64).reshape(len(c), 4, 4)
        sms = [Submap(id=int(s), time=float(c.time[s]), segments=(), pose_flu=np.array(c.pose_flu[s], dtype=np.float64),
                      pose_flu_gt=None if gt is None else gt[s].copy()) for s in keep[r]]
        pos.append(np.stack([np.array(sm.position) for sm in sms]))
        pos_gt.append(None if gt is None else np.stack([np.array(sm.position_gt) for sm in sms]))
        if sm_io.gt_available[r]:
            T_w.append(np.stack([np.array(_read_times(sm, "pose_gravity_aligned_gt", "pose_flu_gt", other[r]), dtype=np.float64) for sm in sms]))
        else:
            T_w.append(np.stack([np.array(_read_times(sm, "pose_gravity_aligned", "pose_flu", other[r]), dtype=np.float64) for sm in sms]))
        times.append(np.array([sm.time for sm in sms], dtype=np.float64))
        frames.append(np.stack([_edge_frames(sm)[r] for sm in sms]))

    # ---- pass 1 on the device: one enqueue, one synchronisation, the pair list and the dense matrices back ----
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f64, i32 = torch.float64, torch.int32
    cap = n0 * n1
    d_in = [dict(pos=up(pos[r]), gt=None if pos_gt[r] is None else up(pos_gt[r]), T_w=up(T_w[r].reshape(-1, 16)), time=up(times[r]),
                 desc=p[r].desc_dev[torch.from_numpy(keep[r].astype(np.int64)).to(dev)].contiguous() if d else None) for r in range(2)]
    d_dist = torch.empty((n0, n1), dtype=f64, device=dev); d_yaw = torch.empty((n0, n1), dtype=f64, device=dev)
    d_sim = torch.empty((n0, n1), dtype=f64, device=dev); d_flags = torch.empty((n0, n1), dtype=i32, device=dev)
    d_Tij = torch.empty((cap, 16), dtype=f64, device=dev); d_Tref = torch.empty((cap, 16), dtype=f64, device=dev)
    d_pairs = torch.empty((cap, 2), dtype=i32, device=dev); d_enable = torch.empty(cap, dtype=i32, device=dev)
    d_ntodo = torch.zeros(1, dtype=i32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    gp = grid_gate_params(sm_params.submap_radius, sm_io.skip_distance, d, sm_params.submap_descriptor_thresh if d else 0.0,
                          sm_params.single_robot_lc, sm_params.single_robot_lc_time_thresh)
    wait_torch()                                             # the uploads are in place before the library's stream reads them
    ctx.grid_gate_dev(gp, n0, n1, ptr(d_in[0]["pos"]), ptr(d_in[0]["T_w"]), ptr(d_in[1]["pos"]), ptr(d_in[1]["T_w"]),
                      d_dist.data_ptr(), d_flags.data_ptr(), d_yaw.data_ptr(), d_sim.data_ptr(), d_Tij.data_ptr(),
                      d_pairs.data_ptr(), d_Tref.data_ptr(), d_enable.data_ptr(), d_ntodo.data_ptr(),
                      time0_ptr=ptr(d_in[0]["time"]), time1_ptr=ptr(d_in[1]["time"]), desc0_ptr=ptr(d_in[0]["desc"]), desc1_ptr=ptr(d_in[1]["desc"]),
                      pos_gt0_ptr=ptr(d_in[0]["gt"]), pos_gt1_ptr=ptr(d_in[1]["gt"]))
    ctx.sync()
    B = int(d_ntodo.cpu().numpy()[0])
    pairs = d_pairs[:B].cpu().numpy().astype(np.int64)
    dist, flags, yaw, sim = d_dist.cpu().numpy(), d_flags.cpu().numpy(), d_yaw.cpu().numpy(), d_sim.cpu().numpy()
    nearby, skip = (flags & _abi.ROMAN_GRID_NEARBY) != 0, (flags & _abi.ROMAN_GRID_SKIP) != 0
    gated, todo = (flags & _abi.ROMAN_GRID_GATED) != 0, (flags & _abi.ROMAN_GRID_TODO) != 0
    robots_nearby_mat[nearby] = dist[nearby]
    T_ij_mat[:] = d_Tij.cpu().numpy().reshape(n0, n1, 4, 4)
    submap_yaw_diff_mat[nearby] = yaw[nearby]
    clipper_num_associations[skip] = 0
    similarity_mat[~skip] = sim[~skip]
    clipper_num_associations[gated] = 0                  # pairs the descriptor gate stopped: the sentinels of [REF :179-184]
    clipper_angle_mat[gated & nearby] = np.abs(np.rad2deg(180.0)); clipper_dist_mat[gated & nearby] = 1e6
    if not np.array_equal(pairs, np.stack(np.nonzero(todo), axis=1)):
        raise _abi.RomanHipError("roman_grid_gate_dev: the compact pair list is not the TODO pairs in row-major order")
    if B == 0:
        return make(empty_edges)
    ti, tj = pairs[:, 0], pairs[:, 1]

    # ---- the hot path over the resident pools: offsets and counts from the pools, the batch in chunks, then the tail ----
    batch, pool = p[0].grid_batch(p[1], mask=todo)
    P = registration._abi_params()
    kmax = batch.kmax()
    a_out = torch.full((B, kmax, 2), -1, dtype=i32, device=dev); n_out = torch.zeros(B, dtype=i32, device=dev)
    T_out = torch.zeros((B, 16), dtype=f64, device=dev); st_out = torch.zeros(B, dtype=i32, device=dev)
    FL, FR = up(frames[0].reshape(-1, 16)), up(frames[1].reshape(-1, 16))
    iL, iR = d_pairs[:B, 0].contiguous(), d_pairs[:B, 1].contiguous()
    records = torch.zeros(B * _abi.LC_RECORD_NBYTES, dtype=torch.uint8, device=dev)
    acc_idx = torch.zeros(B, dtype=i32, device=dev); acc_n = torch.zeros(1, dtype=i32, device=dev)
    lp = LcInputs(dim=sm_params.dim, force_rm_upside_down=sm_params.force_rm_upside_down,
                  force_rm_lc_roll_pitch=sm_params.force_rm_lc_roll_pitch,
                  tilt_thresh=registration.roll_pitch_thresh if getattr(registration, "use_gravity", False) else None,
                  lc_association_thresh=int(np.ceil(sm_io.lc_association_thresh)) if device_edges else 1).params()
    wait_torch()                                             # the pool (torch.cat), the cleared outputs and the frames are in place
    t0 = time.time()
    status = issue_chunked(ctx, P, pool, batch, kmax, a_out, n_out, T_out, st_out)     # re-issues skipped problems, then synchronises:
    ctx.join()                                               # ... the tail below sees the FINAL attempt of every problem only
    ctx.lc_tail_dev(lp, B, T_out.data_ptr(), n_out.data_ptr(), st_out.data_ptr(), records.data_ptr(), acc_idx.data_ptr(), acc_n.data_ptr(),
                    T_ref_ptr=d_Tref.data_ptr(), enable_ptr=d_enable.data_ptr(), FL_ptr=FL.data_ptr(), iL_ptr=iL.data_ptr(),
                    FR_ptr=FR.data_ptr(), iR_ptr=iR.data_ptr())
    ctx.sync()
    timing_list = [(time.time() - t0) / B] * B
    rec = np.frombuffer(records.cpu().numpy().tobytes(), dtype=lc_record_dtype()).copy()
    n_h, a_h = n_out.cpu().numpy(), a_out.cpu().numpy()
    s = sm_params.dim + 1
    res = LoopClosureResult([a_h[b, :n_h[b]].copy() for b in range(B)], T_out.cpu().numpy()[:, :s * s].reshape(B, s, s).copy(), status,
                            np.zeros(B, dtype=stats_dtype()), rec, acc_idx.cpu().numpy()[:int(acc_n.cpu().numpy()[0])].copy())
    lc_edges = _records_into_results(res, ti, tj, nearby, device_edges, clipper_angle_mat, clipper_dist_mat, clipper_num_associations,
                                     T_ij_hat_mat, associated_objs_mat)
    return make(lc_edges, timing_list)


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
            sm = submaps[r][k]
            before = np.array(sm.pose_flu, dtype=np.float64).tobytes()
            for _ in range(n):                           # (stops at the fixed point a yaw-only pose is)
                sm.pose_gravity_aligned
                now = np.array(sm.pose_flu, dtype=np.float64).tobytes()
                if now == before:
                    break
                before = now
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
