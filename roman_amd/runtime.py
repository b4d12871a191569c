"""Thin Python wrapper over the C ABI of libroman_hip.so (include/roman_hip.h).

Everything numerical happens in the HIP library; this module only marshals NumPy arrays (or
device pointers of torch tensors) across ctypes.  There is no CPU fallback: creating a Context
without a gfx950 device raises RomanHipError.
"""
import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _abi
from ._abi import RomanHipError, RomanLcParams, RomanParams, RomanStats


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _vp(x):
    """A device address (an integer; 0 or None: absent) as a ctypes pointer argument."""
    return C.c_void_p(int(x)) if x else None


def _given(a, shape, dtype, fill):
    """An output array of a host-pointer call: the caller's, checked, or a fresh one filled with `fill`."""
    if a is None:
        return np.full(shape, fill, dtype=dtype)
    if a.dtype != dtype or not a.flags.c_contiguous or a.shape != shape:
        raise ValueError(f"an output array must be C-contiguous {np.dtype(dtype).name} of shape {shape}")
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# What the batch wrappers of Context share ("Python side of the entry points"): a wrapper reads "convert, allocate, call, unpack", and each of
# these is one of those steps.  tests/test_runtime_marshalling.py holds what reaches the C ABI through them.
# ---------------------------------------------------------------------------------------------------------------------------
def _vps(*ptrs):
    """Device addresses as pointer arguments, in the order given."""
    return [_vp(p) for p in ptrs]


def _problems(off1, n1, off2, n2):
    """The problem table of a batch call in the C ABI's types -> (off1, n1, off2, n2, B)."""
    off1 = np.ascontiguousarray(off1, dtype=np.int64); off2 = np.ascontiguousarray(off2, dtype=np.int64)
    n1 = np.ascontiguousarray(n1, dtype=np.int32); n2 = np.ascontiguousarray(n2, dtype=np.int32)
    return off1, n1, off2, n2, int(n1.shape[0])


def _pool(feats):
    """A host feature pool -> (feats float64 (n_objects, F), n_objects, F)."""
    feats = _f64(feats)
    if feats.ndim != 2:
        raise ValueError("feats must be (n_objects, F)")
    return (feats, *feats.shape)


def _assoc_list(assoc, assoc_off):
    """Explicit association lists of a host-pointer call (absent: both as they are)."""
    if assoc is None:
        return assoc, assoc_off
    return np.ascontiguousarray(assoc, dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(assoc_off, dtype=np.int64)


def _assoc_off(assoc_off):
    """The offsets of association lists that are in HBM (a device-pointer call)."""
    return None if assoc_off is None else np.ascontiguousarray(assoc_off, dtype=np.int64)


def default_kmax(n1, n2):
    """The association rows a problem of a CLIPPER batch can return: the smaller map of the largest problem (at least 1)."""
    return int(max(1, np.max(np.minimum(n1, n2)))) if len(n1) else 1


def ransac_kmax(n1, n2):
    """The same for a RANSAC batch: every correspondence may be an inlier."""
    return int(max(1, np.max(n1.astype(np.int64) * n2))) if len(n1) else 1


def _ransac_counts(counts, B, rparams):
    """The `counts` argument of the RANSAC calls: None, True (a fresh (B, max_iteration) array of -2) or the caller's, checked."""
    if counts is True:
        return np.full((B, max(int(rparams.max_iteration), 0)), -2, dtype=np.int32)
    if counts is not None and (counts.dtype != np.int32 or not counts.flags.c_contiguous or counts.shape != (B, int(rparams.max_iteration))):
        raise ValueError("counts must be a C-contiguous (B, max_iteration) int32 array")
    return counts


def _solver_out(B, kmax):
    """The cleared host outputs of a single-solution call -> (assoc_out, n_assoc_out, T_out, status_out, stats_out)."""
    stats = np.zeros(B, dtype=stats_dtype())
    assert stats.dtype.itemsize == _abi.STATS_NBYTES
    return np.zeros((B, kmax, 2), dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 16), dtype=np.float64), np.zeros(B, dtype=np.int32), stats


def _mno_out(B, K, kmax):
    """The cleared host outputs of a call with K solutions per problem -> (assoc_out, sol_out, stats_out)."""
    sol = np.zeros((B, K), dtype=mno_solution_dtype())
    assert sol.dtype.itemsize == _abi.MNO_SOLUTION_NBYTES
    return np.zeros((B, K, kmax, 2), dtype=np.int32), sol, np.zeros((B, K), dtype=stats_dtype())


def _tail_out(*shape):
    """The cleared host outputs of the loop-closure tail over (B,) or (B, K) poses -> (records, accepted_idx, n_accepted)."""
    records = np.zeros(shape, dtype=lc_record_dtype())
    assert records.dtype.itemsize == _abi.LC_RECORD_NBYTES
    return records, np.zeros(max(records.size, 1), dtype=np.int32), np.zeros(1, dtype=np.int32)


def _mno_best_out(B):
    """What the hypothesis tail adds per problem -> (best, accepted_best_idx, n_accepted_best)."""
    return np.full(max(B, 1), -1, dtype=np.int32), np.zeros(max(B, 1), dtype=np.int32), np.zeros(1, dtype=np.int32)


def _lc_host_args(lp, arrays):
    """The tail's inputs of a host-pointer call in the C ABI's order: `lp` an LcInputs.params(), `arrays` its arrays(B) — both
    held by the caller until the call has returned."""
    T_ref, enable, FL, iL, FR, iR = arrays
    return [C.byref(lp), _ptr(T_ref), _ptr(enable), _ptr(FL), 0 if FL is None else FL.shape[0], _ptr(iL),
            _ptr(FR), 0 if FR is None else FR.shape[0], _ptr(iR)]


def _solver_result(a_out, n_out, T, dim):
    """-> (the association rows of every problem, the (dim+1)^2 poses) out of the cleared-and-filled outputs, as copies."""
    B, s = T.shape[0], dim + 1
    return [a_out[b, :n_out[b]].copy() for b in range(B)], T[:, :s * s].reshape(B, s, s).copy()


def _mno_result(a_out, sol, K, dim):
    """-> (assoc[b][k], score, T, status) of a call with K solutions per problem, as copies."""
    B, s = sol.shape[0], dim + 1
    return ([[a_out[b, k, :sol["n_assoc"][b, k]].copy() for k in range(K)] for b in range(B)],
            sol["score"].copy(), sol["T"][:, :, :s * s].reshape(B, K, s, s).copy(), sol["status"].copy())


def stats_dtype():
    return np.dtype([("n_assoc_in", np.int32), ("n_live", np.int32), ("nnz_upper", np.int64),
                     ("n_pass", np.int32), ("outer_iters", np.int32), ("inner_iters", np.int32),
                     ("ls_trials", np.int32), ("score", np.float64), ("d_final", np.float64)])


@dataclass
class BatchResult:
    """Results of one batched call, one entry per problem."""
    assoc: list            # list of (k_b, 2) int32 arrays (map-1 index, map-2 index), clipperpy order
    T: np.ndarray          # (B, dim+1, dim+1) float64, NaN where status has INSUFFICIENT/EMPTY_MAP
    status: np.ndarray     # (B,) int32 ROMAN_ST_* flags
    stats: np.ndarray      # (B,) structured array (stats_dtype)


def lc_record_dtype():
    """roman_lc_record_t as a structured dtype."""
    return np.dtype([("problem", np.int32), ("n_assoc", np.int32), ("flags", np.int32), ("reserved", np.int32),
                     ("T_hat", np.float64, (4, 4)), ("theta", np.float64), ("dist", np.float64),
                     ("edge_t", np.float64, (3,)), ("edge_q", np.float64, (4,))])


@dataclass
class LcInputs:
    """What the loop-closure tail needs besides the batch outputs (roman_lc_tail_dev in include/roman_hip.h): the switches of
    roman_lc_params_t and the optional per-problem / per-submap arrays."""
    dim: int = 3
    force_rm_upside_down: bool = False
    force_rm_lc_roll_pitch: bool = False
    tilt_thresh: Optional[float] = None          # radians; None = no tilt check
    lc_association_thresh: int = 4
    T_ref: Optional[np.ndarray] = None           # (B, 4, 4) reference transforms
    enable: Optional[np.ndarray] = None          # (B,) non-zero = may be accepted
    FL: Optional[np.ndarray] = None              # (S0, 4, 4) per-submap frames of the left side, with iL (B,)
    iL: Optional[np.ndarray] = None
    FR: Optional[np.ndarray] = None              # (S1, 4, 4) and iR (B,) for the right side
    iR: Optional[np.ndarray] = None

    def params(self):
        p = RomanLcParams()
        p.dim = int(self.dim)
        p.force_rm_upside_down = int(bool(self.force_rm_upside_down))
        p.force_rm_lc_roll_pitch = int(bool(self.force_rm_lc_roll_pitch))
        p.lc_association_thresh = int(self.lc_association_thresh)
        p.tilt_thresh = -1.0 if self.tilt_thresh is None else float(self.tilt_thresh)
        return p

    def arrays(self, B):
        """The optional arrays in the C ABI's layouts (None stays None)."""
        T_ref = None if self.T_ref is None else _f64(self.T_ref).reshape(B, 16)
        enable = None if self.enable is None else np.ascontiguousarray(self.enable, dtype=np.int32).reshape(B)
        FL = None if self.FL is None else _f64(self.FL).reshape(-1, 16)
        FR = None if self.FR is None else _f64(self.FR).reshape(-1, 16)
        iL = None if self.iL is None else np.ascontiguousarray(self.iL, dtype=np.int32).reshape(B)
        iR = None if self.iR is None else np.ascontiguousarray(self.iR, dtype=np.int32).reshape(B)
        if (FL is None) != (iL is None) or (FR is None) != (iR is None):
            raise ValueError("a frame pool and its index array come together (FL with iL, FR with iR)")
        return T_ref, enable, FL, iL, FR, iR


def mno_solution_dtype():
    """roman_mno_solution_t as a structured dtype."""
    return np.dtype([("n_assoc", np.int32), ("status", np.int32), ("score", np.float64), ("T", np.float64, (16,))])


@dataclass
class MnoResult:
    """Results of one batched multi-solution call: K solutions per problem."""
    assoc: list            # assoc[b][k]: (n, 2) int32 array of solution k of problem b, clipperpy order
    score: np.ndarray      # (B, K) float64 Rayleigh quotient on the unmasked M (0 for an empty selection)
    T: np.ndarray          # (B, K, dim+1, dim+1) float64, NaN where status has INSUFFICIENT / EMPTY_MAP
    status: np.ndarray     # (B, K) int32 ROMAN_ST_* flags
    stats: np.ndarray      # (B, K) structured array (stats_dtype): the statistics of every solve


def ransac_record_dtype():
    """roman_ransac_record_t as a structured dtype (the C compiler's padding included)."""
    return np.dtype({"names": ["n_assoc", "status", "n_hyp", "n_scored", "best_hyp", "best_count", "best_sse", "T"],
                     "formats": [np.int32, np.int32, np.int64, np.int64, np.int64, np.int32, np.float64, (np.float64, (16,))],
                     "offsets": [getattr(_abi.RomanRansacRecord, f).offset for f, _ in _abi.RomanRansacRecord._fields_],
                     "itemsize": _abi.RANSAC_RECORD_NBYTES})


@dataclass
class RansacResult:
    """Results of one batched RANSAC call, one entry per problem."""
    assoc: list            # list of (k_b, 2) int32 arrays: the winner's inliers (map-1 index, map-2 index), row-major order
    T: np.ndarray          # (B, 4, 4) float64 map 2 -> map 1, NaN where status has INSUFFICIENT / EMPTY_MAP
    status: np.ndarray     # (B,) int32 ROMAN_ST_* flags
    records: np.ndarray    # (B,) structured array (ransac_record_dtype)
    counts: Optional[np.ndarray] = None   # (B, max_iteration) int32 when asked for: inlier count per processed hypothesis, -1 = pruned


def submap_desc_dtype():
    """roman_submap_desc_t as a structured dtype."""
    return np.dtype([("pos", np.float64, (3,)), ("T_center_odom", np.float64, (4, 4)), ("time", np.float64),
                     ("t_hi", np.float64), ("t_lo", np.float64)])


@dataclass
class SubmapsResult:
    """Results of one roman_submaps call: fixed slots of `cap` rows per submap, submap s owns rows [s * cap, s * cap + count[s])."""
    pool: Optional[np.ndarray]     # (S * cap, point_dim + F - 3) float64, or None when not asked for
    count: np.ndarray              # (S,) int32
    src: np.ndarray                # (S * cap,) int32 map index of every row
    ids: Optional[np.ndarray]      # (S * cap,) int64, or None without seg_ids
    status: np.ndarray             # (S,) int32: ROMAN_ST_OK / ROMAN_ST_ASSOC_TRUNCATED
    desc: Optional[np.ndarray]     # (S, desc_dim) float64 mean_semantic descriptors, or None


@dataclass
class GridGateResult:
    """Results of one roman_grid_gate call over an S0 x S1 grid: dense matrices and the compact list of the TODO pairs."""
    dist: np.ndarray       # (S0, S1) float64
    flags: np.ndarray      # (S0, S1) int32 ROMAN_GRID_* bits
    yaw_deg: np.ndarray    # (S0, S1) float64, NaN where the pair is not nearby
    sim: np.ndarray        # (S0, S1) float64 (+inf without descriptors)
    T_ij: np.ndarray       # (S0, S1, 4, 4) float64
    pairs: np.ndarray      # (S0 * S1, 2) int32: the first n_todo rows are the TODO pairs, row-major; the others as handed in
    T_ref: np.ndarray      # (S0 * S1, 4, 4) float64, likewise
    enable: np.ndarray     # (S0 * S1,) int32, likewise
    n_todo: int


@dataclass
class SessionGateResult:
    """Results of one roman_session_gate call over the blocks of a session: block b's dense values lie row-major at pair_off[b]."""
    dist: np.ndarray       # (total,) float64
    flags: np.ndarray      # (total,) int32 ROMAN_GRID_* bits
    yaw_deg: np.ndarray    # (total,) float64, NaN where the pair is not nearby
    sim: np.ndarray        # (total,) float64 (+inf without descriptors)
    T_ij: np.ndarray       # (total, 4, 4) float64
    pairs: np.ndarray      # (total, 2) int32: the first todo_off[-1] rows are the TODO pairs as GLOBAL submap indices; the others as handed in
    T_ref: np.ndarray      # (total, 4, 4) float64, likewise
    enable: np.ndarray     # (total,) int32, likewise
    todo_off: np.ndarray   # (nb + 1,) int32: block b's TODO pairs are the compact slots [todo_off[b], todo_off[b + 1])
    pair_off: np.ndarray   # (nb + 1,) int64

    def block(self, b, n0, n1):
        """The dense outputs of block b as (n0, n1) matrices -> dict(dist, flags, yaw_deg, sim, T_ij)."""
        lo, hi = int(self.pair_off[b]), int(self.pair_off[b + 1])
        return dict(dist=self.dist[lo:hi].reshape(n0, n1), flags=self.flags[lo:hi].reshape(n0, n1), yaw_deg=self.yaw_deg[lo:hi].reshape(n0, n1),
                    sim=self.sim[lo:hi].reshape(n0, n1), T_ij=self.T_ij[lo:hi].reshape(n0, n1, 4, 4))


def session_tables(counts, blocks):
    """The small tables of roman_session_gate from the robots' submap counts and the block list [(r0, r1, self_lc), ...] ->
    (sub_off int32 (R + 1,), blocks int32 (nb, 4), pair_off int64 (nb + 1,), tile_off int64 (nb + 1,))."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    sub_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    blk = np.zeros((len(blocks), 4), dtype=np.int32)
    for b, (r0, r1, self_lc) in enumerate(blocks):
        blk[b, :3] = (int(r0), int(r1), int(bool(self_lc)))
    n0, n1 = counts[blk[:, 0]], counts[blk[:, 1]]
    pair_off = np.concatenate([[0], np.cumsum(n0 * n1)]).astype(np.int64)
    tile_off = np.concatenate([[0], np.cumsum(n0 * ((n1 + _abi.GRID_TJ - 1) // _abi.GRID_TJ))]).astype(np.int64)
    return sub_off, blk, pair_off, tile_off


def session_pair_list(counts, blocks, touched):
    """The pair list of roman_session_gate_list from the robots' submap counts, the block list [(r0, r1, ...), ...] and one bool
    array per robot: every pair (i, j) of every block with submap i of r0 touched or submap j of r1 touched -> int32 (L, 3) rows
    (b, i, j), strictly ascending.  touched[r] None: none of robot r's submaps."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    flag = [np.zeros(int(n), dtype=bool) if t is None else np.asarray(t, dtype=bool).reshape(-1) for n, t in zip(counts, touched)]
    if len(flag) != len(counts) or any(len(f) != n for f, n in zip(flag, counts)):
        raise ValueError("touched must hold one flag per submap of every robot")
    rows = []
    for b, blk in enumerate(blocks):
        i, j = np.nonzero(flag[int(blk[0])][:, None] | flag[int(blk[1])][None, :])       # (row-major: ascending in (i, j))
        rows.append(np.stack([np.full(len(i), b, dtype=np.int64), i, j], axis=1))
    return (np.concatenate(rows) if rows else np.zeros((0, 3))).astype(np.int32).reshape(-1, 3)


@dataclass
class SessionGateListResult:
    """Results of one roman_session_gate_list call: entry l belongs to the pair list[l] = (block, i, j)."""
    list: np.ndarray       # (L, 3) int32
    dist: np.ndarray       # (L,) float64
    flags: np.ndarray      # (L,) int32 ROMAN_GRID_* bits
    yaw_deg: np.ndarray    # (L,) float64, NaN where the pair is not nearby
    sim: np.ndarray        # (L,) float64 (+inf without descriptors; with sim_in the pair's entry of it)
    T_ij: np.ndarray       # (L, 4, 4) float64
    pairs: np.ndarray      # (L, 2) int32: the first todo_off[-1] rows are the TODO pairs as GLOBAL submap indices; the others as handed in
    T_ref: np.ndarray      # (L, 4, 4) float64, likewise
    enable: np.ndarray     # (L,) int32, likewise
    todo_off: np.ndarray   # (nb + 1,) int32: block b's TODO pairs are the compact slots [todo_off[b], todo_off[b + 1])


@dataclass
class FrameSelectResult:
    """Results of one roman_frame_select call over the S submaps of a pool and the Nf frames of its map."""
    mask: np.ndarray       # (S, ceil(Nf / 64)) uint64: bit f % 64 of word f / 64
    n_sel: np.ndarray      # (S,) int32
    span: np.ndarray       # (S, 2) float64: min first_seen, max last_seen of the submap's rows ((+inf, -inf) for an empty one)
    mean: Optional[np.ndarray]     # (S, d) float64 with want_mean (NaN rows where nothing is selected), else None

    def selected(self, s):
        """Ascending frame indices of submap s."""
        return mask_indices(self.mask[s])


def mask_indices(words):
    """uint64 mask words -> the ascending indices of the set bits."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    return np.nonzero(bits)[0].astype(np.int64)


def frame_select_params(thin_dist=None, want_mean=False):
    """-> roman_frame_select_params_t (thin_dist None: every candidate frame is selected)."""
    P = _abi.RomanFrameSelectParams()
    P.thin = int(thin_dist is not None)
    P.thin_dist = float(thin_dist) if thin_dist is not None else 0.0
    P.want_mean = int(bool(want_mean))
    return P


def segment_shape_params(center_ref="mean", out_stride=3, col_center=0, col_pca=-1, col_volume=-1, col_extent=-1):
    """-> roman_segment_shape_params_t.  center_ref: 'mean' / 'bottom_middle' [REF roman/object/segment.py:266-274] or a
    ROMAN_CENTER_* number; a column of -1 is not written."""
    P = _abi.RomanSegmentShapeParams()
    if isinstance(center_ref, str):
        if center_ref not in _abi.CENTER_REFS:
            raise ValueError(f"center_ref must be one of {sorted(_abi.CENTER_REFS)} (got {center_ref!r})")
        center_ref = _abi.CENTER_REFS[center_ref]
    P.center_ref, P.out_stride = int(center_ref), int(out_stride)
    P.col_center, P.col_pca, P.col_volume, P.col_extent = int(col_center), int(col_pca), int(col_volume), int(col_extent)
    return P


def _segment_clouds(points, seg_off):
    """The clouds of a host-pointer call in the C ABI's types -> (points float64 (P, 3), seg_off int64 (N + 1,), N)."""
    points = _f64(points)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64).reshape(-1)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must be (P, 3)")
    if seg_off.shape[0] < 1 or int(seg_off[-1]) != points.shape[0]:
        raise ValueError("seg_off must hold N + 1 offsets and end at the number of points")
    return points, seg_off, int(seg_off.shape[0]) - 1


def assoc_params(voxel_size=0.2, geometric="iou", semantic=False, geo_range=(0.25, 1.0), sem_range=(0.8, 1.0)):
    """-> roman_assoc_params_t; the defaults are MapperParams' [REF roman/params/mapper_params.py:58-72].  geometric: 'iou' / 'iom'
    or a ROMAN_ASSOC_* number ('chamfer' is not covered: ValueError); semantic: whether the cosine of the descriptors is the
    second criterion."""
    P = _abi.RomanAssocParams()
    if isinstance(geometric, str):
        if geometric not in _abi.ASSOC_GEOMETRIC:
            raise ValueError(f"geometric must be one of {sorted(_abi.ASSOC_GEOMETRIC)} (got {geometric!r})")
        geometric = _abi.ASSOC_GEOMETRIC[geometric]
    P.voxel_size, P.geometric, P.semantic = float(voxel_size), int(geometric), int(bool(semantic))
    P.geo_range[0], P.geo_range[1] = (float(x) for x in geo_range)
    P.sem_range[0], P.sem_range[1] = (float(x) for x in sem_range)
    return P


@dataclass
class AssocScores:
    """What roman_assoc_scores* writes: geo, sem (None without the cosine), score (N1, N2) float64; inter (N1, N2) int32;
    n_vox and status (clouds,) int32, the row clouds first."""
    geo: np.ndarray
    sem: Optional[np.ndarray]
    score: np.ndarray
    n_vox: Optional[np.ndarray]
    inter: Optional[np.ndarray]
    status: np.ndarray


def _assoc_sizes(clouds, N1, N2, desc):
    """The counts and descriptors of an association call, checked -> (N1, N2, columns, desc float64 (clouds, d) or None, d)."""
    N1, N2 = int(N1), int(N2)
    if N1 < 0 or N2 < -1 or (N1 if N2 < 0 else N1 + N2) != clouds:
        raise ValueError(f"cloud_off holds {clouds} clouds: N1 + N2 must be that (N2 = -1: self mode, N1 alone)")
    d = 0
    if desc is not None:
        desc = _f64(desc)
        if desc.ndim != 2 or desc.shape[0] != clouds:
            raise ValueError(f"desc must be ({clouds}, d)")
        d = int(desc.shape[1])
        if d == 0:
            desc = None
    return N1, N2, (N1 if N2 < 0 else N2), desc, d


def integrate_params(voxel_size=0.05, outlier_std=1.0):
    """-> roman_integrate_params_t; the defaults are MapperParams' segment_voxel_size and segment_outlier_removal_std
    [REF roman/params/mapper_params.py:73-74].  outlier_std None, not finite or <= 0: no outlier removal [REF :100-103]."""
    P = _abi.RomanIntegrateParams()
    P.voxel_size = float(voxel_size)
    P.outlier_std = 0.0 if outlier_std is None else float(outlier_std)
    P.nb_neighbors = _abi.ROMAN_INTEGRATE_NEIGHBORS
    return P


def integrate_jobs(jobs):
    """The job table of a segment update in the C ABI's type: rows (base, add) or (base, add, pose); None stands for -1."""
    rows = [tuple(-1 if v is None else int(v) for v in j) for j in jobs]
    out = np.zeros(len(rows), dtype=_abi.INTEGRATE_JOB_DTYPE)
    for k, r in enumerate(rows):
        if len(r) not in (2, 3):
            raise ValueError("a job is (base, add) or (base, add, pose)")
        out[k] = (r[0], r[1], r[2] if len(r) == 3 else -1)
    return out


def integrate_slots(cloud_off, jobs):
    """The slot offsets of a job table (n_jobs + 1,): the exclusive prefix sum of n(base) + n(add) — where roman_segment_integrate*
    puts every job's output."""
    n = np.diff(np.asarray(cloud_off, dtype=np.int64))
    size = [(int(n[j["base"]]) if j["base"] >= 0 else 0) + int(n[j["add"]]) for j in jobs]
    return np.concatenate([[0], np.cumsum(size, dtype=np.int64)]).astype(np.int64)


@dataclass
class IntegrateOutput:
    """What roman_segment_integrate writes: points (total, 3) and avg (total,) by slot, count / status (n_jobs,) int32, thr
    (n_jobs,), slot (n_jobs + 1,).  avg and thr are None when not asked for."""
    points: np.ndarray
    count: np.ndarray
    status: np.ndarray
    avg: Optional[np.ndarray]
    thr: Optional[np.ndarray]
    slot: np.ndarray

    def cloud(self, j):
        """Job j's cleaned cloud (count, 3)."""
        return self.points[self.slot[j]:self.slot[j] + self.count[j]]


def cluster_params(eps=0.25, min_points=_abi.ROMAN_CLUSTER_MIN_POINTS):
    """-> roman_cluster_params_t; the defaults are MapperParams' clustering_epsilon [REF roman/params/mapper_params.py:68] and
    final_cleanup's min_points [REF roman/object/segment.py:195]."""
    P = _abi.RomanClusterParams()
    P.eps, P.min_points = float(eps), int(min_points)
    return P


def cluster_slots(cloud_off, jobs):
    """The slot offsets of a clustering job list (n_jobs + 1,): the exclusive prefix sum of the jobs' point counts — where
    roman_segment_cluster* puts every job's output."""
    n = np.diff(np.asarray(cloud_off, dtype=np.int64))
    size = [int(n[int(j)]) for j in np.asarray(jobs, dtype=np.int64).reshape(-1)]
    return np.concatenate([[0], np.cumsum(size, dtype=np.int64)]).astype(np.int64)


@dataclass
class ClusterOutput:
    """What roman_segment_cluster writes: points (total, 3) and label (total,) int32 by slot; count, status, n_clusters, kept
    (n_jobs,) int32; slot (n_jobs + 1,).  label and kept are None when not asked for."""
    points: np.ndarray
    count: np.ndarray
    status: np.ndarray
    label: Optional[np.ndarray]
    n_clusters: np.ndarray
    kept: Optional[np.ndarray]
    slot: np.ndarray

    def cloud(self, j):
        """Job j's kept cluster (count, 3), in input order."""
        return self.points[self.slot[j]:self.slot[j] + self.count[j]]

    def labels(self, j):
        """open3d's label of every input point of job j (n,)."""
        return self.label[self.slot[j]:self.slot[j + 1]]


def session_frame_robot_dtype():
    """roman_session_frame_robot_t as a structured dtype."""
    return np.dtype([("seg0", np.int64), ("mask_off", np.int64), ("n_seg", np.int32), ("sub0", np.int32), ("n_sub", np.int32), ("frame0", np.int32),
                     ("n_frames", np.int32), ("mask_words", np.int32), ("reserved", np.int32, (2,))])


def session_frame_robots(n_seg, n_sub, n_frames, mask_words=None):
    """The robots' records of a session whose tables hold every robot's range next to the one in front of it -> a
    session_frame_robot_dtype array (mask_words: per robot, default ceil(Nf_r / 64))."""
    n_seg, n_sub, n_frames = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (n_seg, n_sub, n_frames))
    words = (n_frames + 63) // 64 if mask_words is None else np.asarray(mask_words, dtype=np.int64).reshape(-1)
    first = lambda n: np.concatenate([[0], np.cumsum(n)[:-1]]) if len(n) else n
    rec = np.zeros(len(n_seg), dtype=session_frame_robot_dtype())
    rec["seg0"], rec["n_seg"], rec["sub0"], rec["n_sub"] = first(n_seg), n_seg, first(n_sub), n_sub
    rec["frame0"], rec["n_frames"], rec["mask_words"], rec["mask_off"] = first(n_frames), n_frames, words, first(n_sub * words)
    return rec


def grid_gate_params(radius, skip_distance=np.inf, desc_dim=0, desc_thresh=0.0, single_robot_lc=False, lc_time_thresh=0.0):
    """-> roman_grid_gate_params_t (a missing radius — None — is passed as -1: roman_grid_gate* answers ROMAN_E_UNSUPPORTED,
    roman_grid_gate_aabb* does not read it)."""
    P = _abi.RomanGridGateParams()
    P.radius = -1.0 if radius is None else float(radius)
    P.skip_distance = float(skip_distance)
    P.desc_dim = int(desc_dim)
    P.desc_thresh = float(desc_thresh)
    P.single_robot_lc = int(bool(single_robot_lc))
    P.lc_time_thresh = float(lc_time_thresh)
    return P


@dataclass
class LoopClosureResult(BatchResult):
    """A batch result with the loop-closure tail behind it."""
    records: np.ndarray    # (B,) structured array (lc_record_dtype)
    accepted: np.ndarray   # (n_accepted,) int32: accepted problems, ascending
    # align_lc_batch_ids only (shared-segment removal in front): the objects of either side that stayed, and the ascending local
    # indices of those objects (problem b's side-1 list from sum over c < b of (n1[c] + n2[c]), its side-2 list n1[b] later)
    n1_kept: Optional[np.ndarray] = None
    n2_kept: Optional[np.ndarray] = None
    keep: Optional[np.ndarray] = None
    # ransac_lc_batch only: the (B,) roman_ransac_record_t array (ransac_record_dtype) behind assoc / T / status; `stats` is zeros there
    ransac_records: Optional[np.ndarray] = None


@dataclass
class MnoLoopClosureResult(MnoResult):
    """A multi-solution result with the hypothesis tail behind it (roman_mno_lc_batch)."""
    n_assoc: np.ndarray        # (B, K) int32: associations of every solution as the solver counted them
    records: np.ndarray        # (B, K) structured array (lc_record_dtype); records[b, k]["problem"] == b * K + k
    best: np.ndarray           # (B,) int32: the hypothesis a problem's results come from, -1 when none qualifies
    accepted: np.ndarray       # (n_accepted,) int32: accepted (b, k) as b * K + k, ascending
    accepted_best: np.ndarray  # (n_accepted_best,) int32: problems whose best hypothesis is accepted, ascending


class Context:
    """One roman_ctx: a HIP device + stream + the library's HBM workspace."""

    def __init__(self, device=0, stream=None):
        self._lib = _abi.load_library()
        self._h = C.c_void_p()
        rc = self._lib.roman_ctx_create(C.byref(self._h), int(device), C.c_void_p(stream) if stream else None)
        if rc != 0:
            msg = self._lib.roman_last_error(None)
            raise RomanHipError(f"roman_ctx_create failed ({rc}): {msg.decode() if msg else ''}")
        self.device = int(device)
        # One context holds ONE stepwise problem (the matrices of the last score()/set_matrix_data()).  Every call
        # that replaces or invalidates it bumps this counter; holders of a problem (the clipperpy shim's CLIPPER
        # objects) remember the value they loaded at and re-send their inputs when it has moved on.
        # The stepwise problem lives in workspace 0 of the library, and the library forgets it (its `last.scored`) in two places:
        # on_next_workspace(), which every solver enqueue goes through (align_batch_dev, align_lc_batch_dev, mno_batch_dev,
        # mno_lc_batch_dev, and the host and resident forms built on them), and every host-pointer call that stages its inputs in
        # workspace 0 (ransac_batch, ransac_lc_batch, the gate / frame-select calls; submaps() and submaps_fill() bump the counter too,
        # although their map table travels through the host mirror: a holder then re-sends once more than it must).  The batch wrappers among these
        # bump the counter in ONE place, _workspace_call(); the stage calls further down bump it themselves.  The pure enqueues
        # that only read and write the caller's device buffers through small descriptor stagings of their own — lc_tail_dev,
        # mno_lc_tail_dev, ransac_batch_dev, ransac_lc_batch_dev, shared_ids_dev, shared_reduce_dev, and the other stage calls'
        # _dev forms — leave workspace 0 alone and do not bump it (they go through _enqueue()).
        self._generation = 0
        self.pipeline_depth = 1                 # what set_pipeline() last set (callers that change it restore it)
        self.wide_teams = -1                    # what set_wide_teams() last set
        self.host_batching = (2048, 3)          # what set_host_batching() last set (the library's defaults)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.roman_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pipeline(self, depth):
        """Batches in flight (1 ... 6), see roman_ctx_set_pipeline in include/roman_hip.h.  With depth 2 the
        results of align_batch_dev calls are complete after sync() (or a device-wide synchronise)."""
        self._check(self._lib.roman_ctx_set_pipeline(self._h, int(depth)), "roman_ctx_set_pipeline")
        self.pipeline_depth = int(depth)

    def sync(self):
        self._check(self._lib.roman_ctx_sync(self._h), "roman_ctx_sync")

    def set_host_batching(self, chunk=2048, depth=3):
        """How align_batch() (host pointers) issues a large batch: more than `chunk` problems go to the device as calls of
        `chunk` problems with `depth` of them in flight (roman_ctx_set_host_batching; depth 1 = one call for everything)."""
        self._check(self._lib.roman_ctx_set_host_batching(self._h, int(chunk), int(depth)), "roman_ctx_set_host_batching")
        self.host_batching = (int(chunk), int(depth))

    def set_wide_teams(self, teams_per_xcd=-1):
        """Team mode of the whole-device solver for large live sets (roman_ctx_set_wide_teams): -1 automatic, 0 never, 1 / 2 / 4
        teams per XCD.  A device-pointer caller that gets ROMAN_ST_INTERNAL records back from a batch with several large live
        sets issues those problems again with 0 (pipeline.issue_chunked does)."""
        self._check(self._lib.roman_ctx_set_wide_teams(self._h, int(teams_per_xcd)), "roman_ctx_set_wide_teams")
        self.wide_teams = int(teams_per_xcd)

    def has_history(self, params, F):
        """Does the library hold a sizing history for this parameter block (roman_ctx_has_history)?  Without one the first of
        several queued calls should be waited for, so that the others size their pools from what it needed."""
        yes = C.c_int32(0)
        self._check(self._lib.roman_ctx_has_history(self._h, C.byref(params), int(F), C.byref(yes)), "roman_ctx_has_history")
        return bool(yes.value)

    def cosine_screen_stats(self):
        """(batches whose cosine stage took the bf16 screen + exact candidates, batches that took the dense product, share of the latest
        screened batch left to the dense kernel) — roman_ctx_cosine_screen_stats."""
        a, b, f = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.roman_ctx_cosine_screen_stats(self._h, C.byref(a), C.byref(b), C.byref(f)), "roman_ctx_cosine_screen_stats")
        return int(a.value), int(b.value), float(f.value)

    def join(self, skip_latest=False, stream=None):
        """Make the context's stream — or `stream` (a hipStream_t handle, e.g. torch.cuda.Stream.cuda_stream) — wait for the
        pipelined batches issued so far (optionally all but the latest)."""
        if stream is None:
            self._check(self._lib.roman_ctx_join(self._h, int(bool(skip_latest))), "roman_ctx_join")
        elif int(stream) == 0:
            # roman_ctx_join_on reads a NULL handle as "the context's own stream" — and 0 is also the handle of the legacy default
            # stream (torch.cuda.default_stream().cuda_stream): the waits would land on the wrong stream and a collective queued on
            # the default stream could read records that are not complete
            raise ValueError("join(stream=0): 0 is the legacy default stream's handle, which the C ABI reads as 'the context's stream'; "
                             "queue the collective on an explicit stream (torch.cuda.Stream) and pass its handle")
        else:
            self._check(self._lib.roman_ctx_join_on(self._h, int(bool(skip_latest)), C.c_void_p(int(stream))), "roman_ctx_join_on")

    def skipped(self, wait=True):
        """Running total of problems that batch calls on this context reported with ROMAN_ST_WORKSPACE
        (roman_ctx_skipped); wait=True synchronises the context first so that every issued batch counts."""
        n = C.c_int64(0)
        self._check(self._lib.roman_ctx_skipped(self._h, int(bool(wait)), C.byref(n)), "roman_ctx_skipped")
        return int(n.value)

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.roman_last_error(self._h)
            err = RomanHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
            err.code = int(rc)                                   # the ROMAN_E_* code
            raise err

    def _workspace_call(self, fn, *args):
        """A batch entry that takes a solver workspace or stages in workspace 0: the stepwise problem is gone (see __init__) -> rc."""
        self._generation += 1
        return getattr(self._lib, fn)(self._h, *args)

    def _enqueue(self, fn, *args):
        """A pure enqueue that leaves the workspaces alone: the call and its check."""
        self._check(getattr(self._lib, fn)(self._h, *args), fn)

    def _finish(self, rc, what, result):
        """The end of a host-result call of the align family: `result()` — and on ROMAN_E_INTERNAL, where the library copied the
        outputs back and its message says which problems have none, the same result on the error's `.result`."""
        if rc == _abi.ROMAN_E_INTERNAL:
            msg = self._lib.roman_last_error(self._h)
            err = RomanHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
            err.result = result()
            raise err
        self._check(rc, what)
        return result()

    # ------------------------------------------------------------------ batched hot path
    def align_batch(self, params, feats, off1, n1, off2, n2, assoc=None, assoc_off=None, u0=None,
                    kmax=None):
        """Host-pointer batch call (roman_align_batch).  feats: (n_objects, F) float64."""
        feats, n_obj, F = _pool(feats)
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc, assoc_off = _assoc_list(assoc, assoc_off)
        u0 = None if u0 is None else _f64(u0)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, n_out, T, status, stats = _solver_out(B, kmax)
        rc = self._workspace_call("roman_align_batch", C.byref(params), B, _ptr(feats), n_obj, _ptr(off1), _ptr(n1),
                                  _ptr(off2), _ptr(n2), F, _ptr(assoc), _ptr(assoc_off), _ptr(u0), kmax,
                                  _ptr(a_out), _ptr(n_out), _ptr(T), _ptr(status), _ptr(stats))
        return self._finish(rc, "roman_align_batch", lambda: BatchResult(*_solver_result(a_out, n_out, T, params.point_dim), status, stats))

    def align_batch_resident(self, params, feats_ptr, F, off1, n1, off2, n2, kmax=None, assoc_ptr=None, assoc_off=None, u0_ptr=None):
        """Inputs in HBM (device pointers as integers, e.g. torch.Tensor.data_ptr()), results on the host
        (roman_align_batch_resident): -> BatchResult.  Synchronous; the library chunks, pipelines and retries like align_batch(),
        and the whole result comes back with one copy."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc_off = _assoc_off(assoc_off)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, n_out, T, status, stats = _solver_out(B, kmax)
        rc = self._workspace_call("roman_align_batch_resident", C.byref(params), B, _vp(feats_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(F), _vp(assoc_ptr), _ptr(assoc_off), _vp(u0_ptr), int(kmax),
                                  _ptr(a_out), _ptr(n_out), _ptr(T), _ptr(status), _ptr(stats))
        return self._finish(rc, "roman_align_batch_resident", lambda: BatchResult(*_solver_result(a_out, n_out, T, params.point_dim), status, stats))

    def align_batch_dev(self, params, feats_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, n_assoc_out_ptr,
                        T_out_ptr, status_out_ptr, stats_out_ptr=None, assoc_ptr=None, assoc_off=None,
                        u0_ptr=None):
        """Device-pointer batch call (roman_align_batch_dev).  Pointers are integers (e.g.
        torch.Tensor.data_ptr()); metadata arrays are host NumPy arrays.  A pure enqueue: nothing is
        waited for or read back; problems that found no workspace come back with ROMAN_ST_WORKSPACE
        (run them again)."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc_off = _assoc_off(assoc_off)
        rc = self._workspace_call("roman_align_batch_dev", C.byref(params), B, _vp(feats_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(F), _vp(assoc_ptr), _ptr(assoc_off), _vp(u0_ptr), int(kmax),
                                  *_vps(assoc_out_ptr, n_assoc_out_ptr, T_out_ptr, status_out_ptr, stats_out_ptr))
        self._check(rc, "roman_align_batch_dev")

    # ------------------------------------------------------------------ multi-solution extraction
    def mno_batch(self, params, feats, off1, n1, off2, n2, num_solutions=2, assoc=None, assoc_off=None, kmax=None):
        """Host-pointer batched mno_clipper (roman_mno_batch): `num_solutions` plain-CLIPPER solves per problem with the
        selected block of M zeroed between them, all on the device.  feats: (n_objects, F) float64.  -> MnoResult."""
        feats, n_obj, F = _pool(feats)
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        K = int(num_solutions)
        assoc, assoc_off = _assoc_list(assoc, assoc_off)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, sol, stats = _mno_out(B, max(K, 0), kmax)
        rc = self._workspace_call("roman_mno_batch", C.byref(params), B, _ptr(feats), n_obj, _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2), F,
                                  _ptr(assoc), _ptr(assoc_off), K, int(kmax), _ptr(a_out), _ptr(sol), _ptr(stats))
        self._check(rc, "roman_mno_batch")
        return MnoResult(*_mno_result(a_out, sol, K, params.point_dim), stats)

    def mno_batch_dev(self, params, feats_ptr, F, off1, n1, off2, n2, num_solutions, kmax, assoc_out_ptr, sol_out_ptr,
                      stats_out_ptr=None, assoc_ptr=None, assoc_off=None):
        """Device-pointer batched mno_clipper (roman_mno_batch_dev): pointers are integers, metadata arrays host NumPy arrays.
        A pure enqueue; skipped problems carry ROMAN_ST_WORKSPACE on every solution (issue them again)."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc_off = _assoc_off(assoc_off)
        rc = self._workspace_call("roman_mno_batch_dev", C.byref(params), B, _vp(feats_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(F), _vp(assoc_ptr), _ptr(assoc_off), int(num_solutions), int(kmax),
                                  *_vps(assoc_out_ptr, sol_out_ptr, stats_out_ptr))
        self._check(rc, "roman_mno_batch_dev")

    def mno_lc_tail_dev(self, lc_params, B, K, sol_ptr, records_ptr, best_ptr, accepted_idx_ptr, n_accepted_ptr, accepted_best_idx_ptr,
                        n_accepted_best_ptr, T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None, FR_ptr=None, iR_ptr=None):
        """The tail over K hypotheses per problem on its own (roman_mno_lc_tail_dev): sol_ptr is roman_mno_solution_t[B][K] in HBM,
        the per-problem inputs are shared by a problem's hypotheses; every pointer a device address (an integer).  A pure enqueue
        on the context's stream."""
        self._enqueue("roman_mno_lc_tail_dev", C.byref(lc_params), int(B), int(K),
                      *_vps(sol_ptr, T_ref_ptr, enable_ptr, FL_ptr, iL_ptr, FR_ptr, iR_ptr, records_ptr, best_ptr,
                            accepted_idx_ptr, n_accepted_ptr, accepted_best_idx_ptr, n_accepted_best_ptr))

    def mno_lc_batch_dev(self, params, feats_ptr, F, off1, n1, off2, n2, num_solutions, kmax, assoc_out_ptr, sol_out_ptr, lc_params,
                         records_ptr, best_ptr, accepted_idx_ptr, n_accepted_ptr, accepted_best_idx_ptr, n_accepted_best_ptr,
                         stats_out_ptr=None, assoc_ptr=None, assoc_off=None, T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None,
                         FR_ptr=None, iR_ptr=None):
        """mno_batch_dev with the hypothesis tail enqueued behind its rounds on the same stream (roman_mno_lc_batch_dev): a pure
        enqueue, complete after sync()."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc_off = _assoc_off(assoc_off)
        rc = self._workspace_call("roman_mno_lc_batch_dev", C.byref(params), B, _vp(feats_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(F), _vp(assoc_ptr), _ptr(assoc_off), int(num_solutions), int(kmax),
                                  *_vps(assoc_out_ptr, sol_out_ptr, stats_out_ptr), C.byref(lc_params),
                                  *_vps(T_ref_ptr, enable_ptr, FL_ptr, iL_ptr, FR_ptr, iR_ptr, records_ptr, best_ptr,
                                        accepted_idx_ptr, n_accepted_ptr, accepted_best_idx_ptr, n_accepted_best_ptr))
        self._check(rc, "roman_mno_lc_batch_dev")

    def mno_lc_batch(self, params, feats, off1, n1, off2, n2, lc, num_solutions=2, assoc=None, assoc_off=None, kmax=None):
        """Host-pointer batched mno_clipper with the hypothesis tail behind it (roman_mno_lc_batch): `lc` is an LcInputs whose
        per-problem arrays have B entries.  -> MnoLoopClosureResult."""
        feats, n_obj, F = _pool(feats)
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        K = int(num_solutions)
        assoc, assoc_off = _assoc_list(assoc, assoc_off)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, sol, stats = _mno_out(B, max(K, 0), kmax)
        records, idx, cnt = _tail_out(B, max(K, 0))
        best, bidx, bcnt = _mno_best_out(B)
        lp, lc_arrays = lc.params(), lc.arrays(B)
        rc = self._workspace_call("roman_mno_lc_batch", C.byref(params), B, _ptr(feats), n_obj, _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2), F,
                                  _ptr(assoc), _ptr(assoc_off), K, int(kmax), _ptr(a_out), _ptr(sol), _ptr(stats),
                                  *_lc_host_args(lp, lc_arrays), _ptr(records), _ptr(best), _ptr(idx), _ptr(cnt), _ptr(bidx), _ptr(bcnt))
        self._check(rc, "roman_mno_lc_batch")
        return MnoLoopClosureResult(*_mno_result(a_out, sol, K, params.point_dim), stats, sol["n_assoc"].copy(), records, best[:B].copy(),
                                    idx[:int(cnt[0])].copy(), bidx[:int(bcnt[0])].copy())

    # ------------------------------------------------------------------ RANSAC registration
    def ransac_batch(self, rparams, pts, off1, n1, off2, n2, kmax=None, counts=None):
        """Host-pointer batched RANSAC registration on object centres (roman_ransac_batch).  rparams: a RomanRansacParams;
        pts: (n_objects, 3) float64.  counts: None, True (a fresh (B, max_iteration) int32 array filled with -2) or such an
        array of the caller's (entries beyond a problem's n_hyp come back untouched).  -> RansacResult."""
        pts = _f64(pts)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("pts must be (n_objects, 3)")
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        if kmax is None:
            kmax = ransac_kmax(n1, n2)
        counts = _ransac_counts(counts, B, rparams)
        a_out = np.zeros((B, kmax, 2), dtype=np.int32)
        rec = np.zeros(B, dtype=ransac_record_dtype())
        rc = self._workspace_call("roman_ransac_batch", C.byref(rparams), B, _ptr(pts), pts.shape[0], _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(kmax), _ptr(a_out), _ptr(rec), _ptr(counts))
        self._check(rc, "roman_ransac_batch")
        rows = np.minimum(rec["n_assoc"], kmax)
        return RansacResult([a_out[b, :rows[b]].copy() for b in range(B)], rec["T"].reshape(B, 4, 4).copy(), rec["status"].copy(), rec, counts)

    def ransac_batch_dev(self, rparams, pts_ptr, off1, n1, off2, n2, kmax, assoc_out_ptr, rec_out_ptr, counts_out_ptr=None):
        """Device-pointer batched RANSAC registration (roman_ransac_batch_dev): pointers are integers, metadata arrays host
        NumPy arrays.  A pure enqueue on the context's stream; complete after sync()."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        self._enqueue("roman_ransac_batch_dev", C.byref(rparams), B, _vp(pts_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                      int(kmax), *_vps(assoc_out_ptr, rec_out_ptr, counts_out_ptr))

    def ransac_lc_batch(self, rparams, rows, off1, n1, off2, n2, lc, kmax=None, counts=None):
        """Host-pointer RANSAC loop closures (roman_ransac_lc_batch): ransac_batch() over `rows` — (n_objects, F)
        float64 with F >= 3, the centre in columns 0-2 and nothing else read — with the loop-closure tail `lc` (an LcInputs, dim 3)
        behind it.  -> LoopClosureResult: assoc, T and status as ransac_batch gives them, `stats` zeros, the roman_ransac_record_t
        array in `ransac_records`."""
        rows = _f64(rows)
        if rows.ndim != 2 or rows.shape[1] < 3:
            raise ValueError("rows must be (n_objects, F) with F >= 3")
        n_obj, F = rows.shape
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        if kmax is None:
            kmax = ransac_kmax(n1, n2)
        counts = _ransac_counts(counts, B, rparams)
        a_out, n_out, T, status, stats = _solver_out(B, kmax)    # (no statistics come back: `stats` stays zeros)
        rec = np.zeros(B, dtype=ransac_record_dtype())
        records, idx, cnt = _tail_out(B)
        lp, lc_arrays = lc.params(), lc.arrays(B)
        rc = self._workspace_call("roman_ransac_lc_batch", C.byref(rparams), B, _ptr(rows), n_obj, F, _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(kmax), _ptr(a_out), _ptr(rec), _ptr(counts), _ptr(T), _ptr(n_out), _ptr(status),
                                  *_lc_host_args(lp, lc_arrays), _ptr(records), _ptr(idx), _ptr(cnt))
        self._check(rc, "roman_ransac_lc_batch")
        return LoopClosureResult(*_solver_result(a_out, n_out, T, 3), status, stats, records, idx[:int(cnt[0])].copy(), ransac_records=rec)

    def ransac_lc_batch_dev(self, rparams, rows_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, rec_out_ptr, T_out_ptr=None, n_assoc_out_ptr=None,
                            status_out_ptr=None, lc_params=None, records_ptr=None, accepted_idx_ptr=None, n_accepted_ptr=None, counts_out_ptr=None,
                            T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None, FR_ptr=None, iR_ptr=None):
        """Device-pointer RANSAC loop closures (roman_ransac_lc_batch_dev): k_ransac over rows of F doubles with the split outputs
        T / n_assoc / status, and — with lc_params (a RomanLcParams; None: no tail) — the tail behind it on the context's stream.
        Pointers are integers, metadata arrays host NumPy arrays.  A pure enqueue; complete after sync()."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        self._enqueue("roman_ransac_lc_batch_dev", C.byref(rparams), B, _vp(rows_ptr), int(F), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                      int(kmax), *_vps(assoc_out_ptr, rec_out_ptr, counts_out_ptr, T_out_ptr, n_assoc_out_ptr, status_out_ptr),
                      None if lc_params is None else C.byref(lc_params),
                      *_vps(T_ref_ptr, enable_ptr, FL_ptr, iL_ptr, FR_ptr, iR_ptr, records_ptr, accepted_idx_ptr, n_accepted_ptr))

    # ------------------------------------------------------------------ submaps from a whole map, and from every map of a session
    @staticmethod
    def _submap_descs(descs):
        descs = np.ascontiguousarray(descs, dtype=submap_desc_dtype()).reshape(-1)
        assert descs.dtype.itemsize == _abi.SUBMAP_DESC_NBYTES
        return descs

    @staticmethod
    def _session_tables(seg_off, sub_off, descs, N=None):
        """The two offset tables and the centres of a session of maps in the C ABI's types, sub_off[R] checked against the centres and
        — with N, the host forms — seg_off[R] against the rows -> (seg_off int64[R+1], sub_off int32[R+1], R, descs)."""
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64).reshape(-1); sub_off = np.ascontiguousarray(sub_off, dtype=np.int32).reshape(-1)
        if seg_off.shape[0] != sub_off.shape[0] or seg_off.shape[0] < 1:
            raise ValueError("seg_off and sub_off must both hold R + 1 entries")
        descs = Context._submap_descs(descs)
        if N is None and int(sub_off[-1]) != int(descs.shape[0]):
            raise ValueError("sub_off[R] must be the number of descs")
        if N is not None and (int(seg_off[-1]) != N or int(sub_off[-1]) != int(descs.shape[0])):
            raise ValueError("seg_off[R] must be the rows of seg_feats and sub_off[R] the number of descs")
        return seg_off, sub_off, int(seg_off.shape[0]) - 1, descs

    @staticmethod
    def _map_tables(sparams, seg_feats, seg_times, seg_ids, descs, desc_dim, seg_off=None, sub_off=None):
        """The map tables of a host-pointer submaps call in the C ABI's types, checked against each other, with the sizes that follow
        from them: seg_feats (N, F), seg_times (N, 2), seg_ids (N,) or None, descs (S,), the offsets of a session (None: one map),
        rows = S * cap, Fo the columns of a pool row, d = desc_dim."""
        seg_feats = _f64(seg_feats); seg_times = _f64(seg_times)
        if seg_feats.ndim != 2 or seg_times.shape != (seg_feats.shape[0], 2):
            raise ValueError("seg_feats must be (N, F) and seg_times (N, 2)")
        N, F = seg_feats.shape
        if seg_ids is not None:
            seg_ids = np.ascontiguousarray(seg_ids, dtype=np.int64).reshape(-1)
            if seg_ids.shape[0] != N:
                raise ValueError("seg_ids must hold one entry per segment")
        R = None
        if seg_off is None:
            descs = Context._submap_descs(descs)
        else:
            seg_off, sub_off, R, descs = Context._session_tables(seg_off, sub_off, descs, N)
        S = int(descs.shape[0])
        return SimpleNamespace(seg_feats=seg_feats, seg_times=seg_times, seg_ids=seg_ids, descs=descs, seg_off=seg_off, sub_off=sub_off, R=R, N=N, F=F, S=S,
                               rows=S * max(int(sparams.cap), 0), Fo=int(sparams.point_dim) + F - 3, d=int(desc_dim))

    @staticmethod
    def _submap_outputs(t, pool, count, src, ids_out, status, desc_out, want_pool=True, in_place=False):
        """The output arrays of a host-pointer submaps call over the tables `t`: the caller's (C-contiguous, the C ABI's shapes and types),
        checked, or fresh ones filled with 0 (pool, count, status), -1 (src, ids) and NaN (descriptors).  in_place (the list form): they
        are the session's current outputs — the four that must exist do, and ids and descriptors are there when they were handed in.
        -> pool, count, src, ids_out, status, desc_out."""
        if in_place and any(a is None for a in (pool, count, src, status)):
            raise ValueError("pool, count, src and status are the session's current outputs: all are needed")
        has_ids, has_desc = (ids_out is not None, desc_out is not None) if in_place else (t.seg_ids is not None, t.d > 0)
        pool = _given(pool, (t.rows, max(t.Fo, 0)), np.float64, 0.0) if (want_pool or pool is not None) else None
        count = _given(count, (t.S,), np.int32, 0)
        src = _given(src, (t.rows,), np.int32, -1)
        status = _given(status, (t.S,), np.int32, 0)
        ids_out = _given(ids_out, (t.rows,), np.int64, -1) if has_ids else None
        desc_out = _given(desc_out, (t.S, t.d), np.float64, np.nan) if has_desc else None
        return pool, count, src, ids_out, status, desc_out

    def submaps(self, sparams, seg_feats, seg_times, descs, seg_ids=None, desc_dim=0, want_pool=True,
                pool=None, src=None, ids_out=None, desc_out=None):
        """Host-pointer submap extraction (roman_submaps): the radius mode of submaps_from_roman_map [REF roman/map/map.py:297-346]
        for the S centres in `descs` (a submap_desc_dtype array) over the map table seg_feats (N, F) / seg_times (N, 2) /
        seg_ids (N,).  sparams: a RomanSubmapParams.  Output arrays may be handed in (C-contiguous, the C ABI's shapes and
        types): what the call leaves untouched comes back as it was; fresh ones are filled with 0 (pool), -1 (src, ids) and
        NaN (descriptors).  -> SubmapsResult."""
        t = self._map_tables(sparams, seg_feats, seg_times, seg_ids, descs, desc_dim)
        pool, count, src, ids_out, status, desc_out = self._submap_outputs(t, pool, None, src, ids_out, None, desc_out, want_pool)
        self._generation += 1
        rc = self._lib.roman_submaps(self._h, C.byref(sparams), t.N, t.F, _ptr(t.seg_feats), _ptr(t.seg_times), _ptr(t.seg_ids), t.S, _ptr(t.descs),
                                     _ptr(pool), _ptr(count), _ptr(src), _ptr(ids_out), _ptr(status), t.d, _ptr(desc_out))
        self._check(rc, "roman_submaps")
        return SubmapsResult(pool, count, src, ids_out, status, desc_out)

    def submaps_dev(self, sparams, N, F, seg_feats_ptr, seg_times_ptr, descs, pool_ptr, count_ptr, src_ptr, status_ptr,
                    seg_ids_ptr=None, ids_out_ptr=None, desc_dim=0, desc_out_ptr=None):
        """Device-pointer submap extraction (roman_submaps_dev): bulk pointers are device addresses (integers), `descs` a host
        submap_desc_dtype array.  A pure enqueue on the context's stream; complete after sync()."""
        descs = self._submap_descs(descs)
        rc = self._lib.roman_submaps_dev(self._h, C.byref(sparams), int(N), int(F), _vp(seg_feats_ptr), _vp(seg_times_ptr), _vp(seg_ids_ptr),
                                         int(descs.shape[0]), _ptr(descs), _vp(pool_ptr), _vp(count_ptr), _vp(src_ptr), _vp(ids_out_ptr),
                                         _vp(status_ptr), int(desc_dim), _vp(desc_out_ptr))
        self._check(rc, "roman_submaps_dev")

    def session_submaps(self, sparams, seg_off, seg_feats, seg_times, sub_off, descs, seg_ids=None, desc_dim=0, want_pool=True,
                        pool=None, src=None, ids_out=None, desc_out=None):
        """Host-pointer submaps of the R maps of a session (roman_session_submaps): submaps() for every map in one
        call.  seg_feats (N, F) / seg_times (N, 2) / seg_ids (N,) are the R map tables concatenated in map order, map r owning the
        rows [seg_off[r], seg_off[r+1]) and the centres descs[sub_off[r]:sub_off[r+1]]; `src` holds map-local indices.  Output
        arrays as for submaps().  -> SubmapsResult over all sub_off[R] submaps."""
        t = self._map_tables(sparams, seg_feats, seg_times, seg_ids, descs, desc_dim, seg_off, sub_off)
        pool, count, src, ids_out, status, desc_out = self._submap_outputs(t, pool, None, src, ids_out, None, desc_out, want_pool)
        self._enqueue("roman_session_submaps", C.byref(sparams), t.R, t.F, _ptr(t.seg_off), _ptr(t.seg_feats), _ptr(t.seg_times), _ptr(t.seg_ids),
                      _ptr(t.sub_off), _ptr(t.descs), _ptr(pool), _ptr(count), _ptr(src), _ptr(ids_out), _ptr(status), t.d, _ptr(desc_out))
        return SubmapsResult(pool, count, src, ids_out, status, desc_out)

    def session_submaps_dev(self, sparams, F, seg_off, seg_feats_ptr, seg_times_ptr, sub_off, descs, pool_ptr, count_ptr, src_ptr, status_ptr,
                            seg_ids_ptr=None, ids_out_ptr=None, desc_dim=0, desc_out_ptr=None):
        """Device-pointer submaps of the R maps of a session (roman_session_submaps_dev): bulk pointers are device addresses
        (integers); seg_off, sub_off and `descs` (a submap_desc_dtype array over all sub_off[R] centres) are host arrays.  A pure
        enqueue on the context's stream; complete after sync()."""
        seg_off, sub_off, R, descs = self._session_tables(seg_off, sub_off, descs)
        self._enqueue("roman_session_submaps_dev", C.byref(sparams), R, int(F), _ptr(seg_off), *_vps(seg_feats_ptr, seg_times_ptr, seg_ids_ptr),
                      _ptr(sub_off), _ptr(descs), *_vps(pool_ptr, count_ptr, src_ptr, ids_out_ptr, status_ptr), int(desc_dim), _vp(desc_out_ptr))

    @staticmethod
    def _submap_list(lst):
        """The listed submaps of a session in the C ABI's type -> int32[L] (strictly ascending is the library's to judge)."""
        return np.ascontiguousarray(lst, dtype=np.int32).reshape(-1)

    def session_submaps_list(self, sparams, seg_off, seg_feats, seg_times, sub_off, descs, lst, pool, count, src, status, seg_ids=None, ids_out=None,
                             desc_dim=0, desc_out=None, want_changed=True):
        """Host-pointer rebuild of the LISTED submaps of a session in place (roman_session_submaps_list): the tables as
        for session_submaps(); `lst` the global submap indices, strictly ascending; pool, count, src, status (and ids_out, desc_out) the
        session's CURRENT outputs (C-contiguous, the C ABI's shapes and types), which the call changes in the listed slots only.
        -> (SubmapsResult over the caller's arrays, changed int32[L] or None)."""
        t = self._map_tables(sparams, seg_feats, seg_times, seg_ids, descs, desc_dim, seg_off, sub_off)
        self._submap_outputs(t, pool, count, src, ids_out, status, desc_out, in_place=True)
        lst = self._submap_list(lst)
        changed = np.zeros(len(lst), dtype=np.int32) if want_changed else None
        self._enqueue("roman_session_submaps_list", C.byref(sparams), t.R, t.F, _ptr(t.seg_off), _ptr(t.seg_feats), _ptr(t.seg_times), _ptr(t.seg_ids),
                      _ptr(t.sub_off), _ptr(t.descs), _ptr(pool), _ptr(count), _ptr(src), _ptr(ids_out), _ptr(status), t.d, _ptr(desc_out),
                      int(len(lst)), _ptr(lst), _ptr(changed))
        return SubmapsResult(pool, count, src, ids_out, status, desc_out), changed

    def session_submaps_list_dev(self, sparams, F, seg_off, seg_feats_ptr, seg_times_ptr, sub_off, descs, lst, pool_ptr, count_ptr, src_ptr, status_ptr,
                                 seg_ids_ptr=None, ids_out_ptr=None, desc_dim=0, desc_out_ptr=None, changed_ptr=None):
        """Device-pointer rebuild of the LISTED submaps of a session in place (roman_session_submaps_list_dev): the arguments of
        session_submaps_dev over the whole session, `lst` the global submap indices (host, strictly ascending) and `changed_ptr` a
        device int32[L] or None.  A pure enqueue on the context's stream; complete after sync()."""
        seg_off, sub_off, R, descs = self._session_tables(seg_off, sub_off, descs)
        lst = self._submap_list(lst)
        self._enqueue("roman_session_submaps_list_dev", C.byref(sparams), R, int(F), _ptr(seg_off), *_vps(seg_feats_ptr, seg_times_ptr, seg_ids_ptr),
                      _ptr(sub_off), _ptr(descs), *_vps(pool_ptr, count_ptr, src_ptr, ids_out_ptr, status_ptr), int(desc_dim), _vp(desc_out_ptr),
                      int(len(lst)), _ptr(lst), _vp(changed_ptr))

    # ------------------------------------------------------------------ pass 1 of a grid of submaps
    def grid_gate(self, gparams, pos0, T_w0, pos1, T_w1, time0=None, time1=None, desc0=None, desc1=None, pos_gt0=None, pos_gt1=None,
                  pairs=None, T_ref=None, enable=None):
        """Host-pointer pass 1 of the pair loop over an S0 x S1 grid (roman_grid_gate, [REF roman/align/submap_align.py:93-149],
        radius mode): gparams a RomanGridGateParams (grid_gate_params()); per side pos (S, 3), T_w (S, 4, 4), optionally time
        (S,), desc (S, desc_dim) and pos_gt (S, 3).  The compact outputs may be handed in (C-contiguous, the C ABI's shapes and
        types): the slots beyond n_todo come back as they were; fresh ones are filled with -1 / NaN / -1.  -> GridGateResult."""
        return self._grid_gate_host("roman_grid_gate", gparams, (pos0, T_w0, time0, desc0, pos_gt0, None), (pos1, T_w1, time1, desc1, pos_gt1, None),
                                    pairs, T_ref, enable)

    def _grid_gate_host(self, fn, gparams, side0, side1, pairs, T_ref, enable, sim_in=None, sim_name="sim_in", has_desc=True, aabb=False):
        """The host-pointer gate behind grid_gate / grid_gate_sim / grid_gate_aabb: a side is (pos, T_w, time, desc, pos_gt, box);
        with sim_in (the similarity is an input) desc is not read.  What the entry `fn` carries: has_desc, a desc per side;
        aabb, the boxes and sim_in behind the outputs (without it a given similarity goes in the sim slot)."""
        side = []
        for pos, T_w, tm, desc, gt, box in (side0, side1):
            pos = _f64(pos).reshape(-1, 3); S = pos.shape[0]
            T_w = _f64(T_w).reshape(-1, 16); box = _f64(box).reshape(-1, 6) if aabb else None
            tm = None if tm is None else _f64(tm).reshape(-1)
            desc = None if (desc is None or sim_in is not None) else (_f64(desc).reshape(S, -1) if S else np.zeros((0, max(int(gparams.desc_dim), 0))))
            gt = None if gt is None else _f64(gt).reshape(-1, 3)
            if T_w.shape[0] != S or (aabb and box.shape[0] != S) or (tm is not None and tm.shape[0] != S) or (gt is not None and gt.shape[0] != S):
                raise ValueError("the per-submap arrays of a side must hold one entry per submap")
            if desc is not None and gparams.desc_dim > 0 and desc.shape[1] != gparams.desc_dim:
                raise ValueError("desc must be (S, desc_dim)")
            side.append((S, pos, gt, T_w, tm, desc, box))
        S0, S1 = side[0][0], side[1][0]
        B = S0 * S1
        if sim_in is not None:
            sim_in = _f64(sim_in)
            if sim_in.shape != (S0, S1):
                raise ValueError(f"{sim_name} must be (S0, S1)")
        pairs = _given(pairs, (B, 2), np.int32, -1); T_ref = _given(T_ref, (B, 4, 4), np.float64, np.nan); enable = _given(enable, (B,), np.int32, -1)
        dist = np.zeros((S0, S1)); flags = np.zeros((S0, S1), dtype=np.int32); yaw = np.zeros((S0, S1))
        sim = np.zeros((S0, S1)) if sim_in is None else None
        T_ij = np.zeros((S0, S1, 4, 4)); n_todo = np.zeros(1, dtype=np.int32)
        self._generation += 1
        ins = [_ptr(a) for s in side for a in s[1:(6 if has_desc else 5)]]
        tail = [_ptr(side[0][6]), _ptr(side[1][6]), _ptr(sim_in)] if aabb else []
        rc = getattr(self._lib, fn)(self._h, C.byref(gparams), S0, S1, *ins, _ptr(dist), _ptr(flags), _ptr(yaw),
                                    _ptr(sim if aabb or sim_in is None else sim_in), _ptr(T_ij), _ptr(pairs), _ptr(T_ref), _ptr(enable), _ptr(n_todo), *tail)
        self._check(rc, fn)
        return GridGateResult(dist, flags, yaw, sim if sim_in is None else sim_in, T_ij, pairs, T_ref, enable, int(n_todo[0]))

    def grid_gate_dev(self, gparams, S0, S1, pos0_ptr, T_w0_ptr, pos1_ptr, T_w1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                      pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr, time0_ptr=None, time1_ptr=None, desc0_ptr=None, desc1_ptr=None,
                      pos_gt0_ptr=None, pos_gt1_ptr=None):
        """Device-pointer pass 1 of the pair loop over an S0 x S1 grid (roman_grid_gate_dev): every pointer a device address (an
        integer, e.g. torch.Tensor.data_ptr()).  A pure enqueue on the context's stream; complete after sync().  T_ref_ptr and
        enable_ptr are what lc_tail_dev / align_lc_batch_dev take for the problems of `pairs`."""
        self._grid_gate_dev("roman_grid_gate_dev", gparams, S0, S1, pos0_ptr, pos_gt0_ptr, T_w0_ptr, time0_ptr, desc0_ptr,
                            pos1_ptr, pos_gt1_ptr, T_w1_ptr, time1_ptr, desc1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                            pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr)

    def _grid_gate_dev(self, fn, gparams, S0, S1, *ptrs):
        """The device-pointer gate behind grid_gate_dev / grid_gate_sim_dev / grid_gate_aabb_dev: `ptrs` in the C function's order."""
        rc = getattr(self._lib, fn)(self._h, C.byref(gparams), int(S0), int(S1), *[_vp(p) for p in ptrs])
        self._check(rc, fn)

    def grid_gate_sim(self, gparams, sim, pos0, T_w0, pos1, T_w1, time0=None, time1=None, pos_gt0=None, pos_gt1=None,
                      pairs=None, T_ref=None, enable=None):
        """grid_gate() on a similarity that is already there (roman_grid_gate_sim): `sim` (S0, S1) is read, never written;
        gparams.desc_dim must be 0.  -> GridGateResult whose sim is the array handed in."""
        return self._grid_gate_host("roman_grid_gate_sim", gparams, (pos0, T_w0, time0, None, pos_gt0, None), (pos1, T_w1, time1, None, pos_gt1, None),
                                    pairs, T_ref, enable, sim_in=_f64(sim), sim_name="sim", has_desc=False)

    def grid_gate_sim_dev(self, gparams, S0, S1, pos0_ptr, T_w0_ptr, pos1_ptr, T_w1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                          pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr, time0_ptr=None, time1_ptr=None, pos_gt0_ptr=None, pos_gt1_ptr=None):
        """grid_gate_dev() on a similarity that is already there (roman_grid_gate_sim_dev): sim_ptr is an INPUT."""
        self._grid_gate_dev("roman_grid_gate_sim_dev", gparams, S0, S1, pos0_ptr, pos_gt0_ptr, T_w0_ptr, time0_ptr,
                            pos1_ptr, pos_gt1_ptr, T_w1_ptr, time1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                            pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr)

    # ------------------------------------------------------------------ pass 1 of every robot pair of a session
    _TILE_OFF = (np.int64, (-1,), " and tile_off")           # the last table of the tile gate: one entry per block and one
    _PAIR_LIST = (np.int32, (-1, 3), None)                   # ... and of the list gate: of any length

    @staticmethod
    def _session_gate_tables(sub_off, blocks, pair_off, last, dtype, shape, per_block):
        """The tables of a session gate as the C entries take them; `last`: tile_off or the pair list, of `dtype` and `shape`, and
        with `per_block` (its name in the refusal) of nb + 1 entries.  -> (sub_off, blocks, pair_off, last, R, nb)."""
        sub_off = np.ascontiguousarray(sub_off, dtype=np.int32).reshape(-1); blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 4)
        pair_off = np.ascontiguousarray(pair_off, dtype=np.int64).reshape(-1); last = np.ascontiguousarray(last, dtype=dtype).reshape(shape)
        R, nb = len(sub_off) - 1, len(blocks)
        if R < 0 or len(pair_off) != nb + 1 or (per_block and len(last) != nb + 1):
            raise ValueError(f"sub_off must hold R + 1 entries, pair_off{per_block or ''} nb + 1")
        return sub_off, blocks, pair_off, last, R, nb

    @staticmethod
    def _session_gate_arrays(gparams, sub_off, pos, T_w, time, desc, pos_gt, has_gt, box, sim_in, n_sim):
        """The per-submap arrays of a session gate, contiguous and checked against the tables: one entry per submap of the session
        (sub_off[R]), has_gt one per robot, sim_in `n_sim` entries -> (pos, T_w, time, desc, pos_gt, has_gt, box, sim_in)."""
        R = len(sub_off) - 1
        pos = _f64(pos).reshape(-1, 3); S = pos.shape[0]
        T_w = _f64(T_w).reshape(-1, 16)
        time = None if time is None else _f64(time).reshape(-1)
        desc = None if desc is None else (_f64(desc).reshape(S, -1) if S else np.zeros((0, max(int(gparams.desc_dim), 0))))
        pos_gt = None if pos_gt is None else _f64(pos_gt).reshape(-1, 3)
        has_gt = None if has_gt is None else np.ascontiguousarray(has_gt, dtype=np.int32).reshape(-1)
        if T_w.shape[0] != S or (time is not None and time.shape[0] != S) or (pos_gt is not None and pos_gt.shape[0] != S) or \
                (has_gt is not None and has_gt.shape[0] != R) or int(sub_off[-1]) != S:
            raise ValueError("the per-submap arrays must hold one entry per submap of the session (sub_off[R]), has_gt one per robot")
        if desc is not None and gparams.desc_dim > 0 and desc.shape[1] != gparams.desc_dim:
            raise ValueError("desc must be (S, desc_dim)")
        if sim_in is not None:
            sim_in = _f64(sim_in).reshape(-1)
            if sim_in.shape[0] != n_sim:
                raise ValueError("sim_in must hold pair_off[nb] entries")
        if box is not None:
            box = _f64(box).reshape(-1, 6)
            if box.shape[0] != S:
                raise ValueError("box must hold one row per submap of the session")
        return pos, T_w, time, desc, pos_gt, has_gt, box, sim_in

    @staticmethod
    def _session_gate_entry(box, sim_in):
        """-> the stem of the C entry that serves (box, sim_in) and what follows its outputs: roman_session_gate_aabb* carries
        both, given or not; roman_session_gate_sim* the similarity alone."""
        if box is not None:
            return "roman_session_gate_aabb", (box, sim_in)
        return ("roman_session_gate", ()) if sim_in is None else ("roman_session_gate_sim", (sim_in,))

    def session_gate(self, gparams, sub_off, blocks, pair_off, tile_off, pos, T_w, time=None, desc=None, pos_gt=None, has_gt=None,
                     pairs=None, T_ref=None, enable=None, sim_in=None, box=None):
        """Host-pointer pass 1 over a list of robot pairs (roman_session_gate): the tables as session_tables() gives them (they are
        passed as they are: the library checks them); pos (S, 3), T_w (S, 4, 4), time (S,), desc (S, desc_dim), pos_gt (S, 3) with
        has_gt (R,) over ALL submaps of the session.  gparams.single_robot_lc is not read: a block's own self_lc is.  The compact
        outputs may be handed in, as grid_gate() takes them.  sim_in (pair_off[nb],): the similarity of every pair is given
        (roman_session_gate_sim; gparams.desc_dim must be 0) and comes back as `sim`.  box (S, 6): the bounding-box gate
        (roman_session_gate_aabb, DESIGN.md §4.16: session_gate_aabb() below).  -> SessionGateResult."""
        sub_off, blocks, pair_off, tile_off, R, nb = self._session_gate_tables(sub_off, blocks, pair_off, tile_off, *self._TILE_OFF)
        B = max(int(pair_off[-1]), 0)
        pos, T_w, time, desc, pos_gt, has_gt, box, sim_in = self._session_gate_arrays(gparams, sub_off, pos, T_w, time, desc, pos_gt, has_gt, box, sim_in, B)
        pairs = _given(pairs, (B, 2), np.int32, -1); T_ref = _given(T_ref, (B, 4, 4), np.float64, np.nan); enable = _given(enable, (B,), np.int32, -1)
        dist = np.zeros(B); flags = np.zeros(B, dtype=np.int32); yaw = np.zeros(B); T_ij = np.zeros((B, 4, 4))
        todo_off = np.zeros(nb + 1, dtype=np.int32)
        self._generation += 1
        given = sim_in is not None
        sim = sim_in.copy() if given else np.zeros(B)        # (a given similarity comes back as `sim`)
        # a given similarity travels behind the outputs: the desc and sim slots are then empty
        fn, tail = self._session_gate_entry(box, sim if given else None)
        rc = getattr(self._lib, fn)(self._h, C.byref(gparams), R, _ptr(sub_off), _ptr(pos), _ptr(pos_gt), _ptr(has_gt), _ptr(T_w), _ptr(time),
                                    None if given else _ptr(desc), nb, _ptr(blocks), _ptr(pair_off), _ptr(tile_off), _ptr(dist), _ptr(flags), _ptr(yaw),
                                    None if given else _ptr(sim), _ptr(T_ij), _ptr(pairs), _ptr(T_ref), _ptr(enable), _ptr(todo_off), *map(_ptr, tail))
        self._check(rc, fn)
        return SessionGateResult(dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off, pair_off)

    def session_gate_dev(self, gparams, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos_ptr, T_w_ptr,
                         dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr, pairs_ptr, T_ref_ptr, enable_ptr, todo_off_ptr,
                         time_ptr=None, desc_ptr=None, pos_gt_ptr=None, has_gt_ptr=None, sim_in_ptr=None, box_ptr=None):
        """Device-pointer pass 1 over a list of robot pairs (roman_session_gate_dev): the tables as host arrays (session_tables();
        the library validates these) AND as device addresses of the same values; every other pointer a device address.  A pure
        enqueue on the context's stream; complete after sync().  pairs_ptr holds GLOBAL submap indices: with frames tabled over
        all submaps of the session, its two columns are lc_tail_dev's iL and iR.  sim_in_ptr: the similarity of every pair is
        given (roman_session_gate_sim_dev): gparams.desc_dim must be 0, desc_ptr is not read, sim_ptr not written.
        box_ptr: the bounding-box gate (roman_session_gate_aabb_dev, DESIGN.md §4.16: session_gate_aabb_dev() below)."""
        sub_off, blocks, pair_off, tile_off, R, nb = self._session_gate_tables(sub_off, blocks, pair_off, tile_off, *self._TILE_OFF)
        fn, tail = self._session_gate_entry(box_ptr, sim_in_ptr)
        rc = getattr(self._lib, fn + "_dev")(self._h, C.byref(gparams), R, _vp(sub_off_ptr), _ptr(sub_off), _vp(pos_ptr), _vp(pos_gt_ptr), _vp(has_gt_ptr),
                                             _vp(T_w_ptr), _vp(time_ptr), _vp(desc_ptr), nb, _vp(blocks_ptr), _ptr(blocks), _vp(pair_off_ptr), _ptr(pair_off),
                                             _vp(tile_off_ptr), _ptr(tile_off), _vp(dist_ptr), _vp(flags_ptr), _vp(yaw_deg_ptr), _vp(sim_ptr), _vp(T_ij_ptr),
                                             _vp(pairs_ptr), _vp(T_ref_ptr), _vp(enable_ptr), _vp(todo_off_ptr), *map(_vp, tail))
        self._check(rc, fn + "_dev")

    # ------------------------------------------------------------------ boxes and the bounding-box gate of a session
    def session_boxes(self, pool, row0, count, T_odom_center):
        """Host-pointer boxes of every submap of a session (roman_session_boxes): pool (rows, F) the concatenated pools, submap g
        its rows [row0[g], row0[g] + count[g]) — in any order, overlapping where two views of a robot name the same rows —,
        T_odom_center (S, 4, 4) -> (S, 6) float64: min x y z, max x y z in the global frame."""
        pool = _f64(pool); row0 = np.ascontiguousarray(row0, dtype=np.int64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        S = int(count.shape[0])
        T = _f64(T_odom_center).reshape(-1, 16)
        if pool.ndim != 2 or row0.shape[0] != S or T.shape[0] != S:
            raise ValueError("pool must be (rows, F), row0 and count (S,) and T_odom_center (S, 4, 4)")
        if S and (count.min() < 0 or row0.min() < 0 or int((row0 + count).max()) > pool.shape[0]):
            raise ValueError("a submap's rows lie outside the pool")
        box = np.zeros((S, 6))
        self._generation += 1
        rc = self._lib.roman_session_boxes(self._h, S, int(pool.shape[1]), _ptr(pool), _ptr(row0), _ptr(count), _ptr(T), _ptr(box))
        self._check(rc, "roman_session_boxes")
        return box

    def session_boxes_dev(self, S, F, pool_ptr, row0_ptr, count_ptr, T_odom_center_ptr, box_ptr):
        """Device-pointer boxes of every submap of a session (roman_session_boxes_dev): row0 int64[S] and count int32[S] on the
        device.  A pure enqueue on the context's stream."""
        rc = self._lib.roman_session_boxes_dev(self._h, int(S), int(F), _vp(pool_ptr), _vp(row0_ptr), _vp(count_ptr), _vp(T_odom_center_ptr), _vp(box_ptr))
        self._check(rc, "roman_session_boxes_dev")

    def session_gate_aabb(self, gparams, box, sub_off, blocks, pair_off, tile_off, pos, T_w, **kw):
        """session_gate() with the bounding-box gate (roman_session_gate_aabb): box (S, 6) as session_boxes() gives them;
        gparams.radius is not read; sim_in as in session_gate().  -> SessionGateResult."""
        return self.session_gate(gparams, sub_off, blocks, pair_off, tile_off, pos, T_w, box=_f64(box).reshape(-1, 6), **kw)

    def session_gate_aabb_dev(self, gparams, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos_ptr, T_w_ptr,
                              dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr, pairs_ptr, T_ref_ptr, enable_ptr, todo_off_ptr, box_ptr, **kw):
        """session_gate_dev() with the bounding-box gate (roman_session_gate_aabb_dev): box_ptr as session_boxes_dev wrote them, over
        all submaps of the session; with sim_in_ptr the similarity is an input.  A pure enqueue on the context's stream."""
        if box_ptr is None:
            raise ValueError("session_gate_aabb_dev needs the boxes")
        self.session_gate_dev(gparams, sub_off, blocks, pair_off, tile_off, sub_off_ptr, blocks_ptr, pair_off_ptr, tile_off_ptr, pos_ptr, T_w_ptr,
                              dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr, pairs_ptr, T_ref_ptr, enable_ptr, todo_off_ptr, box_ptr=box_ptr, **kw)

    # ------------------------------------------------------------------ pass 1 of a session over an explicit pair list
    def session_gate_list(self, gparams, sub_off, blocks, pair_off, pair_list, pos, T_w, time=None, desc=None, pos_gt=None, has_gt=None,
                          pairs=None, T_ref=None, enable=None, sim_in=None, box=None):
        """Host-pointer pass 1 over a pair list (roman_session_gate_list): the tables as session_tables() gives them (without
        tile_off), pair_list (L, 3) rows (block, i, j) as session_pair_list() cuts them — both passed as they are: the library
        checks them; the per-submap arrays as session_gate() takes them.  sim_in (pair_off[nb],): the similarity of every pair
        of every block, dense; box (S, 6): the bounding-box gate.  The compact outputs may be handed in.  -> SessionGateListResult."""
        sub_off, blocks, pair_off, pair_list, R, nb = self._session_gate_tables(sub_off, blocks, pair_off, pair_list, *self._PAIR_LIST)
        pos, T_w, time, desc, pos_gt, has_gt, box, sim_in = self._session_gate_arrays(
            gparams, sub_off, pos, T_w, time, None if sim_in is not None else desc, pos_gt, has_gt, box, sim_in, max(int(pair_off[-1]), 0))
        L = len(pair_list)
        pairs = _given(pairs, (L, 2), np.int32, -1); T_ref = _given(T_ref, (L, 4, 4), np.float64, np.nan); enable = _given(enable, (L,), np.int32, -1)
        dist = np.zeros(L); flags = np.zeros(L, dtype=np.int32); yaw = np.zeros(L); sim = np.zeros(L); T_ij = np.zeros((L, 4, 4))
        todo_off = np.zeros(nb + 1, dtype=np.int32)
        self._generation += 1
        rc = self._lib.roman_session_gate_list(self._h, C.byref(gparams), R, _ptr(sub_off), _ptr(pos), _ptr(pos_gt), _ptr(has_gt), _ptr(T_w), _ptr(time),
                                               _ptr(desc), nb, _ptr(blocks), _ptr(pair_off), L, _ptr(pair_list), _ptr(box), _ptr(sim_in), _ptr(dist), _ptr(flags),
                                               _ptr(yaw), _ptr(sim), _ptr(T_ij), _ptr(pairs), _ptr(T_ref), _ptr(enable), _ptr(todo_off))
        self._check(rc, "roman_session_gate_list")
        return SessionGateListResult(pair_list, dist, flags, yaw, sim, T_ij, pairs, T_ref, enable, todo_off)

    def session_gate_list_dev(self, gparams, sub_off, blocks, pair_off, pair_list, sub_off_ptr, blocks_ptr, pair_off_ptr, list_ptr, pos_ptr, T_w_ptr,
                              dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr, pairs_ptr, T_ref_ptr, enable_ptr, todo_off_ptr,
                              time_ptr=None, desc_ptr=None, pos_gt_ptr=None, has_gt_ptr=None, sim_in_ptr=None, box_ptr=None):
        """Device-pointer pass 1 over a pair list (roman_session_gate_list_dev): the tables and the list as host arrays (the library
        validates these) AND as device addresses of the same values; every other pointer a device address.  The dense outputs
        hold L entries, in list order; the compact ones have capacity L.  sim_in_ptr: the similarity of every pair of every
        block at its dense position (what session_stacked_sim_dev writes); box_ptr: the bounding-box gate.  A pure enqueue on
        the context's stream; complete after sync()."""
        sub_off, blocks, pair_off, pair_list, R, nb = self._session_gate_tables(sub_off, blocks, pair_off, pair_list, *self._PAIR_LIST)
        rc = self._lib.roman_session_gate_list_dev(self._h, C.byref(gparams), R, _vp(sub_off_ptr), _ptr(sub_off), _vp(pos_ptr), _vp(pos_gt_ptr), _vp(has_gt_ptr),
                                                   _vp(T_w_ptr), _vp(time_ptr), _vp(desc_ptr), nb, _vp(blocks_ptr), _ptr(blocks), _vp(pair_off_ptr), _ptr(pair_off),
                                                   len(pair_list), _vp(list_ptr), _ptr(pair_list), _vp(box_ptr), _vp(sim_in_ptr), _vp(dist_ptr), _vp(flags_ptr),
                                                   _vp(yaw_deg_ptr), _vp(sim_ptr), _vp(T_ij_ptr), _vp(pairs_ptr), _vp(T_ref_ptr), _vp(enable_ptr), _vp(todo_off_ptr))
        self._check(rc, "roman_session_gate_list_dev")

    # ------------------------------------------------------------------ the stacked similarity of every block of a session
    @staticmethod
    def _session_stacked_tables(frame_lo, frame_n, mask_off, sub_off, blocks, pair_off):
        frame_lo = np.ascontiguousarray(frame_lo, dtype=np.int32).reshape(-1); frame_n = np.ascontiguousarray(frame_n, dtype=np.int32).reshape(-1)
        mask_off = np.ascontiguousarray(mask_off, dtype=np.int64).reshape(-1)
        sub_off = np.ascontiguousarray(sub_off, dtype=np.int32).reshape(-1); blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 4)
        pair_off = np.ascontiguousarray(pair_off, dtype=np.int64).reshape(-1)
        R, nb = len(sub_off) - 1, len(blocks)
        if R < 0 or len(pair_off) != nb + 1 or not (len(frame_lo) == len(frame_n) == len(mask_off) == R):
            raise ValueError("sub_off must hold R + 1 entries, frame_lo, frame_n and mask_off R, pair_off nb + 1")
        return frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, R, nb

    def session_stacked_sim(self, desc, mask, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off):
        """Host-pointer stacked similarity of every block of a session (roman_session_stacked_sim): desc (Nf, d) the ONE frame
        table, mask the uint64 words of all views' frame masks, view r = frames [frame_lo[r], frame_lo[r] + frame_n[r]) with its
        masks (n_r, ceil(frame_n[r] / 64)) at word mask_off[r]; sub_off, blocks, pair_off as session_tables() gives them.
        -> sim (pair_off[nb],) float64, block b row-major at pair_off[b]."""
        desc = _f64(desc)
        if desc.ndim != 2:
            raise ValueError("session_stacked_sim needs an (Nf, d) frame table")
        mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(-1)
        frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, R, nb = self._session_stacked_tables(frame_lo, frame_n, mask_off, sub_off, blocks, pair_off)
        sim = np.zeros(max(int(pair_off[-1]), 0))
        self._generation += 1
        rc = self._lib.roman_session_stacked_sim(self._h, desc.shape[1], desc.shape[0], _ptr(desc), _ptr(mask), mask.shape[0], R, _ptr(frame_lo), _ptr(frame_n),
                                                 _ptr(mask_off), _ptr(sub_off), nb, _ptr(blocks), _ptr(pair_off), _ptr(sim))
        self._check(rc, "roman_session_stacked_sim")
        return sim

    def session_stacked_sim_dev(self, d, Nf, desc_ptr, mask_ptr, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off,
                                frame_lo_ptr, frame_n_ptr, mask_off_ptr, sub_off_ptr, blocks_ptr, pair_off_ptr, sim_ptr):
        """Device-pointer stacked similarity of every block of a session (roman_session_stacked_sim_dev): the tables as host arrays
        (the library validates these) AND as device addresses of the same values; desc, mask and sim device addresses.  A pure
        enqueue on the context's stream: session_gate_dev(..., sim_in_ptr=sim_ptr) behind it reads what it wrote."""
        frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, R, nb = self._session_stacked_tables(frame_lo, frame_n, mask_off, sub_off, blocks, pair_off)
        rc = self._lib.roman_session_stacked_sim_dev(self._h, int(d), int(Nf), _vp(desc_ptr), _vp(mask_ptr), R, _vp(frame_lo_ptr), _ptr(frame_lo),
                                                     _vp(frame_n_ptr), _ptr(frame_n), _vp(mask_off_ptr), _ptr(mask_off), _vp(sub_off_ptr), _ptr(sub_off),
                                                     nb, _vp(blocks_ptr), _ptr(blocks), _vp(pair_off_ptr), _ptr(pair_off), _vp(sim_ptr))
        self._check(rc, "roman_session_stacked_sim_dev")

    # ------------------------------------------------------------------ ... and of a list of its pairs
    def session_stacked_sim_list(self, desc, mask, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, pair_list, sim=None):
        """Host-pointer stacked similarity of a LIST of pairs of a session (roman_session_stacked_sim_list): session_stacked_sim()'s
        arguments, then pair_list (L, 3) int32 rows (b, i, j) as session_pair_list() builds them, strictly ascending.  `sim`
        (pair_off[nb],): the dense array the listed entries are written into — the others come back as they were; None: NaN.
        -> sim (pair_off[nb],) float64: a listed pair at pair_off[b] + i * n1 + j, bit for bit session_stacked_sim()'s entry."""
        desc = _f64(desc)
        if desc.ndim != 2:
            raise ValueError("session_stacked_sim_list needs an (Nf, d) frame table")
        mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(-1)
        frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, R, nb = self._session_stacked_tables(frame_lo, frame_n, mask_off, sub_off, blocks, pair_off)
        pair_list = np.ascontiguousarray(pair_list, dtype=np.int32).reshape(-1, 3)
        sim = _given(sim, (max(int(pair_off[-1]), 0),), np.float64, np.nan)
        self._generation += 1
        rc = self._lib.roman_session_stacked_sim_list(self._h, desc.shape[1], desc.shape[0], _ptr(desc), _ptr(mask), mask.shape[0], R, _ptr(frame_lo),
                                                      _ptr(frame_n), _ptr(mask_off), _ptr(sub_off), nb, _ptr(blocks), _ptr(pair_off), len(pair_list),
                                                      _ptr(pair_list), _ptr(sim))
        self._check(rc, "roman_session_stacked_sim_list")
        return sim

    def session_stacked_sim_list_dev(self, d, Nf, desc_ptr, mask_ptr, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, pair_list,
                                     frame_lo_ptr, frame_n_ptr, mask_off_ptr, sub_off_ptr, blocks_ptr, pair_off_ptr, list_ptr, sim_ptr):
        """Device-pointer stacked similarity of a list of pairs (roman_session_stacked_sim_list_dev): session_stacked_sim_dev()'s
        arguments with the list as a host array (validated) AND as a device address, as session_gate_list_dev takes it.  Writes
        the listed pairs' entries of the DENSE array at sim_ptr and nothing else.  A pure enqueue on the context's stream:
        session_gate_list_dev(..., sim_in_ptr=sim_ptr) behind it reads what it wrote."""
        frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, R, nb = self._session_stacked_tables(frame_lo, frame_n, mask_off, sub_off, blocks, pair_off)
        pair_list = np.ascontiguousarray(pair_list, dtype=np.int32).reshape(-1, 3)
        rc = self._lib.roman_session_stacked_sim_list_dev(self._h, int(d), int(Nf), _vp(desc_ptr), _vp(mask_ptr), R, _vp(frame_lo_ptr), _ptr(frame_lo),
                                                          _vp(frame_n_ptr), _ptr(frame_n), _vp(mask_off_ptr), _ptr(mask_off), _vp(sub_off_ptr), _ptr(sub_off),
                                                          nb, _vp(blocks_ptr), _ptr(blocks), _vp(pair_off_ptr), _ptr(pair_off), len(pair_list), _vp(list_ptr),
                                                          _ptr(pair_list), _vp(sim_ptr))
        self._check(rc, "roman_session_stacked_sim_list_dev")

    # ------------------------------------------------------------------ force-fill submaps, boxes, the bounding-box gate
    def submaps_fill(self, point_dim, cap, seg_feats, descs, count, src, seg_ids=None, desc_dim=0, want_pool=True):
        """Host-pointer gather of force-fill submaps (roman_submaps_fill, [REF roman/map/map.py:264-295]): `src` (S, cap) holds the
        map indices of every submap's rows (the first count[s] of a row are read), `descs` a submap_desc_dtype array whose
        T_center_odom takes the centres to the submap's frame.  -> SubmapsResult (count and src are the arrays handed in; status 0)."""
        seg_feats = _f64(seg_feats)
        if seg_feats.ndim != 2:
            raise ValueError("seg_feats must be (N, F)")
        N, F = seg_feats.shape
        if seg_ids is not None:
            seg_ids = np.ascontiguousarray(seg_ids, dtype=np.int64).reshape(-1)
            if seg_ids.shape[0] != N:
                raise ValueError("seg_ids must hold one entry per segment")
        descs = self._submap_descs(descs)
        S, cap, d = int(descs.shape[0]), int(cap), int(desc_dim)
        count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        if count.shape[0] != S or src.shape[0] != S * max(cap, 0):
            raise ValueError("count must be (S,) and src (S, cap)")
        rows, Fo = S * max(cap, 0), int(point_dim) + F - 3
        pool = np.zeros((rows, max(Fo, 0))) if want_pool else None
        ids_out = np.full(rows, -1, dtype=np.int64) if seg_ids is not None else None
        desc_out = np.full((S, d), np.nan) if d > 0 else None
        self._generation += 1
        rc = self._lib.roman_submaps_fill(self._h, int(point_dim), cap, N, F, _ptr(seg_feats), _ptr(seg_ids), S, _ptr(descs), _ptr(count), _ptr(src),
                                          _ptr(pool), _ptr(ids_out), d, _ptr(desc_out))
        self._check(rc, "roman_submaps_fill")
        return SubmapsResult(pool, count, src, ids_out, np.zeros(S, dtype=np.int32), desc_out)

    def submaps_fill_dev(self, point_dim, cap, N, F, seg_feats_ptr, descs, count_ptr, src_ptr, pool_ptr, seg_ids_ptr=None, ids_out_ptr=None,
                         desc_dim=0, desc_out_ptr=None):
        """Device-pointer gather of force-fill submaps (roman_submaps_fill_dev): count and src are device arrays the caller uploaded,
        `descs` a host submap_desc_dtype array.  A pure enqueue on the context's stream; complete after sync()."""
        descs = self._submap_descs(descs)
        rc = self._lib.roman_submaps_fill_dev(self._h, int(point_dim), int(cap), int(N), int(F), _vp(seg_feats_ptr), _vp(seg_ids_ptr), int(descs.shape[0]),
                                              _ptr(descs), _vp(count_ptr), _vp(src_ptr), _vp(pool_ptr), _vp(ids_out_ptr), int(desc_dim), _vp(desc_out_ptr))
        self._check(rc, "roman_submaps_fill_dev")

    def submap_boxes(self, pool, cap, count, T_odom_center):
        """Host-pointer boxes of the submaps of a pool (roman_submap_boxes, [REF roman/map/map.py:133-139]): pool (S * cap, F),
        count (S,), T_odom_center (S, 4, 4) -> (S, 6) float64: min x y z, max x y z in the global frame."""
        pool = _f64(pool); count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        S, cap = int(count.shape[0]), int(cap)
        T = _f64(T_odom_center).reshape(-1, 16)
        if pool.ndim != 2 or pool.shape[0] != S * max(cap, 0) or T.shape[0] != S:
            raise ValueError("pool must be (S * cap, F), count (S,) and T_odom_center (S, 4, 4)")
        if S and (count.min() < 0 or count.max() > cap):
            raise ValueError("a count lies outside [0, cap]")
        box = np.zeros((S, 6))
        self._generation += 1
        rc = self._lib.roman_submap_boxes(self._h, S, int(pool.shape[1]), cap, _ptr(pool), _ptr(count), _ptr(T), _ptr(box))
        self._check(rc, "roman_submap_boxes")
        return box

    def submap_boxes_dev(self, S, F, cap, pool_ptr, count_ptr, T_odom_center_ptr, box_ptr):
        """Device-pointer boxes of the submaps of a pool (roman_submap_boxes_dev): a pure enqueue on the context's stream."""
        rc = self._lib.roman_submap_boxes_dev(self._h, int(S), int(F), int(cap), _vp(pool_ptr), _vp(count_ptr), _vp(T_odom_center_ptr), _vp(box_ptr))
        self._check(rc, "roman_submap_boxes_dev")

    # ------------------------------------------------------------------ segment tables from point clouds
    def segment_shapes(self, points, seg_off, sparams, out=None):
        """Host-pointer centre and shape features of every segment of a map from its points (roman_segment_shapes): points (P, 3),
        seg_off (N + 1,) ascending from 0 to P, sparams a segment_shape_params() block.  `out` (N, sparams.out_stride) float64: the
        caller's table — the columns the block does not name come back as they were — or None for a fresh table of zeros.
        -> (out, status (N,) int32 of ROMAN_SEG_* flags)."""
        points, seg_off, N = _segment_clouds(points, seg_off)
        out = _given(out, (N, int(sparams.out_stride)), np.float64, 0.0)
        status = np.zeros(N, dtype=np.int32)
        self._generation += 1
        rc = self._lib.roman_segment_shapes(self._h, _ptr(points), _ptr(seg_off), N, C.byref(sparams), _ptr(out), _ptr(status))
        self._check(rc, "roman_segment_shapes")
        return out, status

    def segment_shapes_dev(self, points_ptr, seg_off_ptr, seg_off, sparams, out_ptr, status_ptr):
        """Device-pointer form (roman_segment_shapes_dev): points, seg_off, out and status on the device, `seg_off` the same offsets
        on the host (the launch is sized from them).  A pure enqueue on the context's stream."""
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64).reshape(-1)
        if seg_off.shape[0] < 1:
            raise ValueError("seg_off must hold N + 1 offsets")
        self._enqueue("roman_segment_shapes_dev", _vp(points_ptr), _vp(seg_off_ptr), _ptr(seg_off), int(seg_off.shape[0]) - 1, C.byref(sparams),
                      _vp(out_ptr), _vp(status_ptr))

    def set_segment_block_min(self, n=0):
        """Measurement only (roman_ctx_set_segment_block_min): the point count from which a segment takes a workgroup; 0: the default."""
        self._check(self._lib.roman_ctx_set_segment_block_min(self._h, int(n)), "roman_ctx_set_segment_block_min")

    # ------------------------------------------------------------------ frame data association scores
    def assoc_scores(self, aparams, points, cloud_off, N1, N2=-1, desc=None, want_sem=True, want_inter=True, want_n_vox=True):
        """Host-pointer voxel IoU / IoM, cosine and score of every (row cloud, column cloud) pair (roman_assoc_scores): points
        (P, 3), cloud_off (clouds + 1,) ascending from 0 to P — the first N1 clouds are the rows, the next N2 the columns; N2 = -1:
        self mode, N1 x N1.  aparams an assoc_params() block; desc (clouds, d) or None.  -> AssocScores (sem None unless the
        block asks for the cosine; inter / n_vox None when not wanted)."""
        points, cloud_off, clouds = _segment_clouds(points, cloud_off)
        N1, N2, cols, desc, d = _assoc_sizes(clouds, N1, N2, desc)
        n_vox = np.zeros(clouds, dtype=np.int32) if want_n_vox else None
        status = np.zeros(clouds, dtype=np.int32)
        inter = np.zeros((N1, cols), dtype=np.int32) if want_inter else None
        geo, score = np.zeros((N1, cols)), np.zeros((N1, cols))
        sem = np.zeros((N1, cols)) if (want_sem and aparams.semantic) else None
        self._generation += 1
        rc = self._lib.roman_assoc_scores(self._h, C.byref(aparams), _ptr(points), _ptr(cloud_off), N1, N2, _ptr(desc), d,
                                          _ptr(n_vox), _ptr(inter), _ptr(geo), _ptr(sem), _ptr(score), _ptr(status))
        self._check(rc, "roman_assoc_scores")
        return AssocScores(geo, sem, score, n_vox, inter, status)

    def assoc_scores_dev(self, aparams, points_ptr, cloud_off_ptr, cloud_off, N1, N2, desc_ptr, d, geo_ptr, score_ptr, status_ptr,
                         sem_ptr=None, inter_ptr=None, n_vox_ptr=None):
        """Device-pointer form (roman_assoc_scores_dev): every array on the device, `cloud_off` the same offsets on the host (the
        launches and the workspace are sized from them).  A pure enqueue on the context's stream."""
        cloud_off = np.ascontiguousarray(cloud_off, dtype=np.int64).reshape(-1)
        clouds = int(N1) if int(N2) < 0 else int(N1) + int(N2)
        if cloud_off.shape[0] != clouds + 1:
            raise ValueError("cloud_off must hold one offset per cloud and the end")
        self._enqueue("roman_assoc_scores_dev", C.byref(aparams), _vp(points_ptr), _vp(cloud_off_ptr), _ptr(cloud_off), int(N1), int(N2), _vp(desc_ptr), int(d),
                      _vp(n_vox_ptr), _vp(inter_ptr), _vp(geo_ptr), _vp(sem_ptr), _vp(score_ptr), _vp(status_ptr))

    def set_assoc_cuts(self, wave_max=0, lds_max=0):
        """Measurement only (roman_ctx_set_assoc_cuts): the point counts up to which a cloud's keys are sorted by one wave / by
        one workgroup in LDS; 0: the default.  Results do not depend on them."""
        self._check(self._lib.roman_ctx_set_assoc_cuts(self._h, int(wave_max), int(lds_max)), "roman_ctx_set_assoc_cuts")

    # ------------------------------------------------------------------ segment update
    def segment_integrate(self, iparams, points, cloud_off, jobs, poses=None, want_avg=False, want_thr=True, out_points=None, out_avg=None, out_thr=None):
        """Host-pointer segment update (roman_segment_integrate): points (P, 3), cloud_off (clouds + 1,), jobs an integrate_jobs()
        table or rows (base, add[, pose]), poses (n_poses, 4, 4) or None; iparams an integrate_params() block.  out_points (total, 3),
        out_avg (total,), out_thr (n_jobs,): arrays of the caller's, whose untouched elements keep their values (fresh ones start
        at 0, the thresholds at NaN).  -> IntegrateOutput."""
        points, cloud_off, clouds = _segment_clouds(points, cloud_off)
        jobs = jobs if isinstance(jobs, np.ndarray) and jobs.dtype == np.dtype(_abi.INTEGRATE_JOB_DTYPE) else integrate_jobs(jobs)
        jobs = np.ascontiguousarray(jobs)
        n_jobs = int(jobs.shape[0])
        if n_jobs and (jobs["add"].min() < 0 or max(jobs["add"].max(), jobs["base"].max()) >= clouds or jobs["base"].min() < -1):
            raise ValueError(f"a job names a cloud outside the {clouds} given")
        n_poses = 0
        if poses is not None:
            poses = _f64(poses)
            if poses.ndim != 3 or poses.shape[1:] != (4, 4):
                raise ValueError("poses must be (n_poses, 4, 4)")
            n_poses = int(poses.shape[0])
        slot = integrate_slots(cloud_off, jobs)
        total = int(slot[-1])
        out_points = _given(out_points, (total, 3), np.float64, 0.0)
        count, status = np.zeros(n_jobs, dtype=np.int32), np.zeros(n_jobs, dtype=np.int32)
        avg = _given(out_avg, (total,), np.float64, 0.0) if (want_avg or out_avg is not None) else None
        thr = _given(out_thr, (n_jobs,), np.float64, np.nan) if (want_thr or out_thr is not None) else None
        self._generation += 1
        rc = self._lib.roman_segment_integrate(self._h, C.byref(iparams), _ptr(points), _ptr(cloud_off), clouds, _ptr(poses), n_poses,
                                               _ptr(jobs), n_jobs, _ptr(out_points), _ptr(count), _ptr(status), _ptr(avg), _ptr(thr))
        self._check(rc, "roman_segment_integrate")
        return IntegrateOutput(out_points, count, status, avg, thr, slot)

    def segment_integrate_dev(self, iparams, points_ptr, cloud_off_ptr, cloud_off, poses_ptr, n_poses, jobs_ptr, jobs, out_points_ptr, out_count_ptr,
                              out_status_ptr, out_avg_ptr=None, out_thr_ptr=None):
        """Device-pointer form (roman_segment_integrate_dev): every array on the device; `cloud_off` and `jobs` (an integrate_jobs()
        table) are the same numbers on the host — the slots, the launches and the workspace are sized from them.  A pure enqueue
        on the context's stream."""
        cloud_off = np.ascontiguousarray(cloud_off, dtype=np.int64).reshape(-1)
        jobs = np.ascontiguousarray(jobs, dtype=_abi.INTEGRATE_JOB_DTYPE)
        self._enqueue("roman_segment_integrate_dev", C.byref(iparams), _vp(points_ptr), _vp(cloud_off_ptr), _ptr(cloud_off), int(cloud_off.shape[0]) - 1,
                      _vp(poses_ptr), int(n_poses), _vp(jobs_ptr), _ptr(jobs), int(jobs.shape[0]), _vp(out_points_ptr), _vp(out_count_ptr),
                      _vp(out_status_ptr), _vp(out_avg_ptr), _vp(out_thr_ptr))

    def set_integrate_cuts(self, wave_max=0, lds_max=0):
        """Measurement only (roman_ctx_set_integrate_cuts): the point counts (base + added) up to which a job is one wave's / is
        sorted by one workgroup in LDS; 0: the default.  Results do not depend on them."""
        self._check(self._lib.roman_ctx_set_integrate_cuts(self._h, int(wave_max), int(lds_max)), "roman_ctx_set_integrate_cuts")

    # ------------------------------------------------------------------ segment clustering
    def segment_cluster(self, cparams, points, cloud_off, jobs, want_labels=True, want_kept=True, out_points=None, out_labels=None):
        """Host-pointer segment clustering (roman_segment_cluster): points (P, 3), cloud_off (clouds + 1,), jobs the cloud index
        of every job; cparams a cluster_params() block.  out_points (total, 3), out_labels (total,): arrays of the caller's, whose
        untouched elements keep their values (fresh ones start at 0, the labels at -1).  -> ClusterOutput."""
        points, cloud_off, clouds = _segment_clouds(points, cloud_off)
        jobs = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1))
        n_jobs = int(jobs.shape[0])
        if n_jobs and (jobs.min() < 0 or jobs.max() >= clouds):
            raise ValueError(f"a job names a cloud outside the {clouds} given")
        slot = cluster_slots(cloud_off, jobs)
        total = int(slot[-1])
        out_points = _given(out_points, (total, 3), np.float64, 0.0)
        count, status, n_clusters = (np.zeros(n_jobs, dtype=np.int32) for _ in range(3))
        label = _given(out_labels, (total,), np.int32, -1) if (want_labels or out_labels is not None) else None
        kept = np.full(n_jobs, -1, dtype=np.int32) if want_kept else None
        self._generation += 1
        rc = self._lib.roman_segment_cluster(self._h, C.byref(cparams), _ptr(points), _ptr(cloud_off), clouds, _ptr(jobs), n_jobs,
                                             _ptr(out_points), _ptr(count), _ptr(status), _ptr(label), _ptr(n_clusters), _ptr(kept))
        self._check(rc, "roman_segment_cluster")
        return ClusterOutput(out_points, count, status, label, n_clusters, kept, slot)

    def segment_cluster_dev(self, cparams, points_ptr, cloud_off_ptr, cloud_off, jobs_ptr, jobs, out_points_ptr, out_count_ptr, out_status_ptr,
                            out_n_clusters_ptr, out_labels_ptr=None, out_kept_ptr=None):
        """Device-pointer form (roman_segment_cluster_dev): every array on the device; `cloud_off` and `jobs` are the same numbers
        on the host — the slots, the launches and the workspace are sized from them.  A pure enqueue on the context's stream."""
        cloud_off = np.ascontiguousarray(cloud_off, dtype=np.int64).reshape(-1)
        jobs = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1))
        self._enqueue("roman_segment_cluster_dev", C.byref(cparams), _vp(points_ptr), _vp(cloud_off_ptr), _ptr(cloud_off), int(cloud_off.shape[0]) - 1,
                      _vp(jobs_ptr), _ptr(jobs), int(jobs.shape[0]), _vp(out_points_ptr), _vp(out_count_ptr), _vp(out_status_ptr),
                      _vp(out_labels_ptr), _vp(out_n_clusters_ptr), _vp(out_kept_ptr))

    def set_cluster_cuts(self, wave_max=0, lds_max=0):
        """Measurement and tests only (roman_ctx_set_cluster_cuts): the point counts up to which a job is one wave's / is held in
        LDS by one workgroup; 0: the default.  Results do not depend on them."""
        self._check(self._lib.roman_ctx_set_cluster_cuts(self._h, int(wave_max), int(lds_max)), "roman_ctx_set_cluster_cuts")

    def grid_gate_aabb(self, gparams, box0, box1, pos0, T_w0, pos1, T_w1, time0=None, time1=None, desc0=None, desc1=None, pos_gt0=None, pos_gt1=None,
                       sim_in=None, pairs=None, T_ref=None, enable=None):
        """grid_gate() with the bounding-box gate (roman_grid_gate_aabb): box_r (S_r, 6) as submap_boxes() gives them; gparams.radius
        is not read.  `sim_in` (S0, S1): the similarity is already there (gparams.desc_dim must be 0); the result's sim is then
        that array.  -> GridGateResult."""
        return self._grid_gate_host("roman_grid_gate_aabb", gparams, (pos0, T_w0, time0, desc0, pos_gt0, box0), (pos1, T_w1, time1, desc1, pos_gt1, box1),
                                    pairs, T_ref, enable, sim_in=sim_in, aabb=True)

    def grid_gate_aabb_dev(self, gparams, S0, S1, pos0_ptr, T_w0_ptr, pos1_ptr, T_w1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                           pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr, box0_ptr=None, box1_ptr=None, sim_in_ptr=None, time0_ptr=None, time1_ptr=None,
                           desc0_ptr=None, desc1_ptr=None, pos_gt0_ptr=None, pos_gt1_ptr=None):
        """grid_gate_dev() with the bounding-box gate (roman_grid_gate_aabb_dev): box_r as submap_boxes_dev wrote them; with
        sim_in_ptr the similarity is an input (sim_ptr is then not written).  A pure enqueue on the context's stream."""
        self._grid_gate_dev("roman_grid_gate_aabb_dev", gparams, S0, S1, pos0_ptr, pos_gt0_ptr, T_w0_ptr, time0_ptr, desc0_ptr,
                            pos1_ptr, pos_gt1_ptr, T_w1_ptr, time1_ptr, desc1_ptr, dist_ptr, flags_ptr, yaw_deg_ptr, sim_ptr, T_ij_ptr,
                            pairs_ptr, T_ref_ptr, enable_ptr, n_todo_ptr, box0_ptr, box1_ptr, sim_in_ptr)

    # ------------------------------------------------------------------ frame descriptors of the submaps of a pool
    def frame_select(self, fparams, count, src, seg_times, frame_times, frame_pos=None, frame_desc=None):
        """Host-pointer frame selection (roman_frame_select, [REF roman/map/map.py:210-242]): count (S,) and src (S, cap) as
        roman_submaps wrote them, seg_times (N, 2), frame_times (Nf,), frame_pos (Nf, 3) for thinning, frame_desc (Nf, d) for the
        mean.  fparams: frame_select_params().  -> FrameSelectResult."""
        count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1); S = count.shape[0]
        src = np.ascontiguousarray(src, dtype=np.int32)
        if src.ndim != 2 or src.shape[0] != S or src.shape[1] < 1:
            raise ValueError("src must be (S, cap)")
        cap = src.shape[1]
        seg_times = _f64(seg_times).reshape(-1, 2)
        frame_times = _f64(frame_times).reshape(-1); Nf = frame_times.shape[0]
        frame_pos = None if frame_pos is None else _f64(frame_pos).reshape(Nf, 3)
        frame_desc = None if frame_desc is None else _f64(frame_desc).reshape(Nf, -1)
        d = 0 if frame_desc is None else frame_desc.shape[1]
        W = (Nf + 63) // 64
        mask = np.zeros((S, W), dtype=np.uint64); n_sel = np.zeros(S, dtype=np.int32); span = np.zeros((S, 2))
        mean = np.full((S, d), np.nan) if fparams.want_mean else None
        self._generation += 1
        rc = self._lib.roman_frame_select(self._h, C.byref(fparams), S, cap, _ptr(count), _ptr(src), seg_times.shape[0], _ptr(seg_times),
                                          Nf, _ptr(frame_times), _ptr(frame_pos), d, _ptr(frame_desc), _ptr(mask), _ptr(n_sel), _ptr(span), _ptr(mean))
        self._check(rc, "roman_frame_select")
        return FrameSelectResult(mask, n_sel, span, mean)

    def frame_select_dev(self, fparams, S, cap, count_ptr, src_ptr, N, seg_times_ptr, Nf, frame_times_ptr, mask_ptr, n_sel_ptr, span_ptr,
                         frame_pos_ptr=None, d=0, frame_desc_ptr=None, mean_ptr=None):
        """Device-pointer frame selection (roman_frame_select_dev): a pure enqueue on the context's stream, behind submaps_dev."""
        rc = self._lib.roman_frame_select_dev(self._h, C.byref(fparams), int(S), int(cap), _vp(count_ptr), _vp(src_ptr), int(N), _vp(seg_times_ptr),
                                              int(Nf), _vp(frame_times_ptr), _vp(frame_pos_ptr), int(d), _vp(frame_desc_ptr),
                                              _vp(mask_ptr), _vp(n_sel_ptr), _vp(span_ptr), _vp(mean_ptr))
        self._check(rc, "roman_frame_select_dev")

    @staticmethod
    def _frame_robots(robots):
        robots = np.ascontiguousarray(robots, dtype=session_frame_robot_dtype()).reshape(-1)
        assert robots.dtype.itemsize == _abi.SESSION_FRAME_ROBOT_NBYTES
        return robots

    def session_frame_select_list(self, fparams, robots, count, src, seg_times, frame_times, lst, mask, n_sel, span, frame_pos=None, frame_desc=None,
                                  mean=None):
        """Host-pointer frame selection of the LISTED slots of a session in place (roman_session_frame_select_list):
        `robots` a session_frame_robot_dtype array; count (S,) and src (S, cap) by global slot; seg_times, frame_times, frame_pos,
        frame_desc the session's tables; mask (uint64 words), n_sel (S,), span (S, 2) and mean (S, d) the session's CURRENT outputs
        (C-contiguous), which the call changes in the listed slots only.  -> changed int32[L]."""
        robots = self._frame_robots(robots)
        count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1); S = count.shape[0]
        src = np.ascontiguousarray(src, dtype=np.int32)
        if src.ndim != 2 or src.shape[0] != S or src.shape[1] < 1:
            raise ValueError("src must be (S, cap)")
        seg_times = _f64(seg_times).reshape(-1, 2); frame_times = _f64(frame_times).reshape(-1); Nf = frame_times.shape[0]
        frame_pos = None if frame_pos is None else _f64(frame_pos).reshape(Nf, 3)
        frame_desc = None if frame_desc is None else _f64(frame_desc).reshape(Nf, -1)
        d = 0 if frame_desc is None else frame_desc.shape[1]
        ends = lambda a, n, per=1: int(max([0] + [int(x) + int(y) * int(z) for x, y, z in zip(robots[a], robots[n], np.broadcast_to(per, robots[n].shape))]))
        if ends("seg0", "n_seg") > seg_times.shape[0] or ends("sub0", "n_sub") > S or ends("frame0", "n_frames") > Nf:
            raise ValueError("a robot's range reaches beyond the session's tables")
        _given(mask, (ends("mask_off", "n_sub", robots["mask_words"]),), np.uint64, 0)
        _given(n_sel, (S,), np.int32, 0); _given(span, (S, 2), np.float64, 0)
        if fparams.want_mean:
            _given(mean, (S, d), np.float64, 0)
        lst = self._submap_list(lst)
        changed = np.zeros(len(lst), dtype=np.int32)
        self._generation += 1
        rc = self._lib.roman_session_frame_select_list(self._h, C.byref(fparams), len(robots), _ptr(robots), src.shape[1], _ptr(count), _ptr(src),
                                                       _ptr(seg_times), _ptr(frame_times), _ptr(frame_pos), d, _ptr(frame_desc), len(lst), _ptr(lst),
                                                       _ptr(mask), _ptr(n_sel), _ptr(span), _ptr(mean) if fparams.want_mean else None, _ptr(changed))
        self._check(rc, "roman_session_frame_select_list")
        return changed

    def session_frame_select_list_dev(self, fparams, robots, cap, count_ptr, src_ptr, seg_times_ptr, frame_times_ptr, lst, mask_ptr, n_sel_ptr, span_ptr,
                                      changed_ptr, frame_pos_ptr=None, d=0, frame_desc_ptr=None, mean_ptr=None):
        """Device-pointer frame selection of the LISTED slots of a session in place (roman_session_frame_select_list_dev): `robots` (a
        session_frame_robot_dtype array) and `lst` (global slots, strictly ascending) are host arrays, everything else a device
        address.  A pure enqueue on the context's stream, behind session_submaps_list_dev."""
        robots = self._frame_robots(robots)
        lst = self._submap_list(lst)
        self._enqueue("roman_session_frame_select_list_dev", C.byref(fparams), len(robots), _ptr(robots), int(cap), *_vps(count_ptr, src_ptr, seg_times_ptr,
                      frame_times_ptr, frame_pos_ptr), int(d), _vp(frame_desc_ptr), int(len(lst)), _ptr(lst), *_vps(mask_ptr, n_sel_ptr, span_ptr, mean_ptr, changed_ptr))

    def stacked_sim(self, desc0, mask0, desc1, mask1):
        """Host-pointer stacked similarity of a grid (roman_stacked_sim, [REF roman/map/map.py:155-162]): desc_r (Nf_r, d) the
        frame descriptors of map r, mask_r (S_r, ceil(Nf_r / 64)) uint64 as frame_select wrote it -> sim (S0, S1)."""
        desc0, desc1 = _f64(desc0), _f64(desc1)
        if desc0.ndim != 2 or desc1.ndim != 2 or desc0.shape[1] != desc1.shape[1]:
            raise ValueError("stacked_sim needs two (Nf, d) frame tables of the same d")
        mask0 = np.ascontiguousarray(mask0, dtype=np.uint64); mask1 = np.ascontiguousarray(mask1, dtype=np.uint64)
        for m, D in ((mask0, desc0), (mask1, desc1)):
            if m.ndim != 2 or m.shape[1] != (D.shape[0] + 63) // 64:
                raise ValueError("a mask must be (S, ceil(Nf / 64))")
        sim = np.zeros((mask0.shape[0], mask1.shape[0]))
        self._generation += 1
        rc = self._lib.roman_stacked_sim(self._h, desc0.shape[1], desc0.shape[0], _ptr(desc0), mask0.shape[0], _ptr(mask0),
                                         desc1.shape[0], _ptr(desc1), mask1.shape[0], _ptr(mask1), _ptr(sim))
        self._check(rc, "roman_stacked_sim")
        return sim

    def stacked_sim_dev(self, d, Nf0, desc0_ptr, S0, mask0_ptr, Nf1, desc1_ptr, S1, mask1_ptr, sim_ptr):
        """Device-pointer stacked similarity of a grid (roman_stacked_sim_dev): a pure enqueue on the context's stream."""
        rc = self._lib.roman_stacked_sim_dev(self._h, int(d), int(Nf0), _vp(desc0_ptr), int(S0), _vp(mask0_ptr), int(Nf1), _vp(desc1_ptr),
                                             int(S1), _vp(mask1_ptr), _vp(sim_ptr))
        self._check(rc, "roman_stacked_sim_dev")

    def set_stacked_band(self, rows=0):
        """Rows of map 0's frames one band of stacked_sim takes (roman_ctx_set_stacked_band): 0 automatic, otherwise rounded up to
        a multiple of _abi.STACKED_BAND_MIN.  The result does not depend on it."""
        self._check(self._lib.roman_ctx_set_stacked_band(self._h, int(rows)), "roman_ctx_set_stacked_band")

    # ------------------------------------------------------------------ loop closures
    def align_lc_batch(self, params, feats, off1, n1, off2, n2, lc, assoc=None, assoc_off=None, u0=None, kmax=None):
        """Host-pointer batch call with the loop-closure tail behind it (roman_align_lc_batch): `lc` is an LcInputs.
        -> LoopClosureResult; one read-back brings outputs, records and the accepted list."""
        feats, n_obj, F = _pool(feats)
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc, assoc_off = _assoc_list(assoc, assoc_off)
        u0 = None if u0 is None else _f64(u0)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, n_out, T, status, stats = _solver_out(B, kmax)
        records, idx, cnt = _tail_out(B)
        lp, lc_arrays = lc.params(), lc.arrays(B)
        rc = self._workspace_call("roman_align_lc_batch", C.byref(params), B, _ptr(feats), n_obj, _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2), F,
                                  _ptr(assoc), _ptr(assoc_off), _ptr(u0), kmax, _ptr(a_out), _ptr(n_out), _ptr(T), _ptr(status), _ptr(stats),
                                  *_lc_host_args(lp, lc_arrays), _ptr(records), _ptr(idx), _ptr(cnt))
        return self._finish(rc, "roman_align_lc_batch", lambda: LoopClosureResult(*_solver_result(a_out, n_out, T, params.point_dim), status, stats,
                                                                                  records, idx[:int(cnt[0])].copy()))

    def align_lc_batch_ids(self, params, feats, ids, off1, n1, off2, n2, lc, assoc=None, assoc_off=None, u0=None, kmax=None, want_keep=True):
        """align_lc_batch() for self loop closures (roman_align_lc_batch_ids): `ids` holds one int64 per row of `feats`; every
        problem first loses the objects whose id occurs on both of its sides — on the device, over the pool that holds every
        submap once.  -> LoopClosureResult with n1_kept, n2_kept (and keep, the kept local indices, unless want_keep is False);
        associations index the reduced maps.  `assoc` must stay None (the library refuses explicit lists together with ids)."""
        feats, n_obj, F = _pool(feats)
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ids.shape[0] != n_obj:
            raise ValueError("ids must hold one entry per row of feats")
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc, assoc_off = _assoc_list(assoc, assoc_off)
        u0 = None if u0 is None else _f64(u0)
        if kmax is None:
            kmax = default_kmax(n1, n2)
        a_out, n_out, T, status, stats = _solver_out(B, kmax)
        records, idx, cnt = _tail_out(B)
        k1 = np.zeros(B, dtype=np.int32); k2 = np.zeros(B, dtype=np.int32)
        keep = np.full(int(n1.sum(dtype=np.int64) + n2.sum(dtype=np.int64)), -1, dtype=np.int32) if want_keep else None
        lp, lc_arrays = lc.params(), lc.arrays(B)
        rc = self._workspace_call("roman_align_lc_batch_ids", C.byref(params), B, _ptr(feats), n_obj, _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2), F,
                                  _ptr(assoc), _ptr(assoc_off), _ptr(u0), kmax, _ptr(a_out), _ptr(n_out), _ptr(T), _ptr(status), _ptr(stats),
                                  *_lc_host_args(lp, lc_arrays), _ptr(records), _ptr(idx), _ptr(cnt), _ptr(ids), _ptr(k1), _ptr(k2), _ptr(keep))
        return self._finish(rc, "roman_align_lc_batch_ids", lambda: LoopClosureResult(*_solver_result(a_out, n_out, T, params.point_dim), status, stats,
                                                                                      records, idx[:int(cnt[0])].copy(), k1, k2, keep))

    def shared_ids_dev(self, B, ids_ptr, off1, n1, off2, n2, keep_ptr, kept_ptr):
        """The mark step of the shared-segment removal on its own (roman_shared_ids_dev): ids, keep and kept are device addresses
        (integers), the offsets and sizes host arrays.  A pure enqueue on the context's stream; complete after sync()."""
        off1, n1, off2, n2, _ = _problems(off1, n1, off2, n2)
        self._enqueue("roman_shared_ids_dev", int(B), _vp(ids_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2), _vp(keep_ptr), _vp(kept_ptr))

    def shared_reduce_dev(self, B, F, feats_ptr, region_row0, ids_ptr, off1, n1, off2, n2, keep_ptr, kept_ptr):
        """Mark and gather of the shared-segment removal in one launch (roman_shared_reduce_dev): feats (the pool's rows, then a
        gather region of sum(n1 + n2) rows from row region_row0 on), ids, keep and kept are device addresses (integers), the
        offsets and sizes host arrays.  A pure enqueue on the context's stream; complete after sync()."""
        off1, n1, off2, n2, _ = _problems(off1, n1, off2, n2)
        self._enqueue("roman_shared_reduce_dev", int(B), int(F), _vp(feats_ptr), int(region_row0), _vp(ids_ptr), _ptr(off1), _ptr(n1),
                      _ptr(off2), _ptr(n2), _vp(keep_ptr), _vp(kept_ptr))

    def lc_tail_dev(self, lc_params, B, T_ptr, n_assoc_ptr, status_ptr, records_ptr, accepted_idx_ptr, n_accepted_ptr,
                    T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None, FR_ptr=None, iR_ptr=None):
        """The tail on its own over batch outputs in HBM (roman_lc_tail_dev): every pointer a device address (an integer, e.g.
        torch.Tensor.data_ptr()); lc_params a RomanLcParams (LcInputs.params()).  A pure enqueue on the context's stream."""
        self._enqueue("roman_lc_tail_dev", C.byref(lc_params), int(B),
                      *_vps(T_ptr, n_assoc_ptr, status_ptr, T_ref_ptr, enable_ptr, FL_ptr, iL_ptr, FR_ptr, iR_ptr,
                            records_ptr, accepted_idx_ptr, n_accepted_ptr))

    def align_lc_batch_dev(self, params, feats_ptr, F, off1, n1, off2, n2, kmax, assoc_out_ptr, n_assoc_out_ptr, T_out_ptr, status_out_ptr,
                           lc_params, records_ptr, accepted_idx_ptr, n_accepted_ptr, stats_out_ptr=None, assoc_ptr=None, assoc_off=None, u0_ptr=None,
                           T_ref_ptr=None, enable_ptr=None, FL_ptr=None, iL_ptr=None, FR_ptr=None, iR_ptr=None):
        """align_batch_dev with the tail enqueued behind the solver on the same stream (roman_align_lc_batch_dev): a pure enqueue,
        complete after sync()."""
        off1, n1, off2, n2, B = _problems(off1, n1, off2, n2)
        assoc_off = _assoc_off(assoc_off)
        rc = self._workspace_call("roman_align_lc_batch_dev", C.byref(params), B, _vp(feats_ptr), _ptr(off1), _ptr(n1), _ptr(off2), _ptr(n2),
                                  int(F), _vp(assoc_ptr), _ptr(assoc_off), _vp(u0_ptr), int(kmax),
                                  *_vps(assoc_out_ptr, n_assoc_out_ptr, T_out_ptr, status_out_ptr, stats_out_ptr), C.byref(lc_params),
                                  *_vps(T_ref_ptr, enable_ptr, FL_ptr, iL_ptr, FR_ptr, iR_ptr, records_ptr, accepted_idx_ptr, n_accepted_ptr))
        self._check(rc, "roman_align_lc_batch_dev")

    # ------------------------------------------------------------------ stepwise (clipperpy shim)
    def score(self, params, D1, D2, assoc=None):
        D1, D2 = _f64(D1), _f64(D2)
        n1, n2 = D1.shape[0], D2.shape[0]
        F = D1.shape[1] if D1.ndim == 2 else 0
        if D2.ndim == 2 and D2.shape[1] != F and n1 > 0 and n2 > 0:
            raise ValueError("D1 and D2 must have the same number of features")
        if n1 == 0 and D2.ndim == 2:
            F = D2.shape[1]
        na = 0
        if assoc is not None:
            assoc = np.ascontiguousarray(assoc, dtype=np.int32).reshape(-1, 2)
            na = assoc.shape[0]
        self._generation += 1
        rc = self._lib.roman_score(self._h, C.byref(params), _ptr(D1), n1, _ptr(D2), n2, F, _ptr(assoc), na)
        self._check(rc, "roman_score")

    def set_matrix_data(self, params, M, Cm):
        M, Cm = _f64(M), _f64(Cm)
        if M.shape != Cm.shape or M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise ValueError("M and C must be square matrices of the same shape")
        self._generation += 1
        self._check(self._lib.roman_set_matrix_data(self._h, C.byref(params), _ptr(M), _ptr(Cm), M.shape[0]),
                    "roman_set_matrix_data")

    def solve(self, u0=None):
        u0a = None if u0 is None else _f64(u0)
        self._check(self._lib.roman_solve(self._h, _ptr(u0a)), "roman_solve")

    def num_associations(self):
        n = C.c_int32(0)
        self._check(self._lib.roman_num_associations(self._h, C.byref(n)), "roman_num_associations")
        return n.value

    def selected_associations(self):
        n = C.c_int32(0)
        self._check(self._lib.roman_num_selected(self._h, C.byref(n)), "roman_num_selected")
        out = np.zeros((max(n.value, 1), 2), dtype=np.int32)
        self._check(self._lib.roman_get_selected_associations(self._h, _ptr(out)), "roman_get_selected_associations")
        return out[:n.value].copy()

    def solution(self):
        """-> (nodes int32 (k,), u float64 (A,), score, RomanStats)"""
        n = C.c_int32(0); na = C.c_int32(0)
        self._check(self._lib.roman_num_selected(self._h, C.byref(n)), "roman_num_selected")
        self._check(self._lib.roman_num_associations(self._h, C.byref(na)), "roman_num_associations")
        nodes = np.zeros(max(n.value, 1), dtype=np.int32)
        u = np.zeros(max(na.value, 1), dtype=np.float64)
        score = C.c_double(0.0); st = RomanStats()
        self._check(self._lib.roman_get_solution(self._h, _ptr(nodes), _ptr(u), C.byref(score), C.byref(st)),
                    "roman_get_solution")
        return nodes[:n.value].copy(), u[:na.value].copy(), score.value, st

    def dense_matrices(self):
        na = self.num_associations()
        M = np.zeros((na, na), dtype=np.float64); Cm = np.zeros((na, na), dtype=np.float64)
        if na > 0:
            self._check(self._lib.roman_get_dense_matrices(self._h, _ptr(M), _ptr(Cm)), "roman_get_dense_matrices")
        return M, Cm

    def upper_csr(self):
        """-> (rowptr int64 (A+1,), cols int32, vals float64, diag float64 (A,))"""
        na = self.num_associations()
        nnz = C.c_int64(0)
        self._check(self._lib.roman_get_upper_csr(self._h, C.byref(nnz), None, None, None, None), "roman_get_upper_csr")
        rowptr = np.zeros(na + 1, dtype=np.int64)
        cols = np.zeros(max(nnz.value, 1), dtype=np.int32); vals = np.zeros(max(nnz.value, 1), dtype=np.float64)
        diag = np.zeros(max(na, 1), dtype=np.float64)
        self._check(self._lib.roman_get_upper_csr(self._h, C.byref(nnz), _ptr(rowptr), _ptr(cols), _ptr(vals), _ptr(diag)),
                    "roman_get_upper_csr")
        return rowptr, cols[:nnz.value].copy(), vals[:nnz.value].copy(), diag[:na].copy()

    def live(self):
        n = C.c_int32(0)
        self._check(self._lib.roman_debug_live(self._h, C.byref(n), None, None), "roman_debug_live")
        idx = np.zeros(max(n.value, 1), dtype=np.int32); sc = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(self._lib.roman_debug_live(self._h, C.byref(n), _ptr(idx), _ptr(sc)), "roman_debug_live")
        return idx[:n.value].copy(), sc[:n.value].copy()

    # ------------------------------------------------------------------ pose
    def pose_batch(self, dim, pts1, pts2, corr_off):
        pts1 = _f64(pts1).reshape(-1, dim); pts2 = _f64(pts2).reshape(-1, dim)
        corr_off = np.ascontiguousarray(corr_off, dtype=np.int64)
        B = corr_off.shape[0] - 1
        T = np.zeros((max(B, 1), 16), dtype=np.float64); status = np.zeros(max(B, 1), dtype=np.int32)
        self._check(self._lib.roman_pose_batch(self._h, int(dim), B, _ptr(pts1), _ptr(pts2), _ptr(corr_off), _ptr(T),
                                               _ptr(status)), "roman_pose_batch")
        s = dim + 1
        return T[:B, :s * s].reshape(B, s, s).copy(), status[:B].copy()

    # ------------------------------------------------------------------ instrumentation / diagnostics
    def profile_enable(self, on=True):
        self._check(self._lib.roman_profile_enable(self._h, int(bool(on))), "roman_profile_enable")

    def profile_reset(self):
        self._check(self._lib.roman_profile_reset(self._h), "roman_profile_reset")

    def profile_get(self):
        ms = (C.c_double * _abi.ROMAN_STAGE_COUNT)(); n = (C.c_int64 * _abi.ROMAN_STAGE_COUNT)()
        self._check(self._lib.roman_profile_get(self._h, ms, n), "roman_profile_get")
        return {name: (ms[i], n[i]) for i, name in enumerate(_abi.STAGE_NAMES)}

    def debug_math(self, kind, x, y=None):
        x = _f64(x).ravel(); ya = None if y is None else _f64(y).ravel()
        out = np.zeros_like(x)
        self._check(self._lib.roman_debug_math(self._h, int(kind), _ptr(x), _ptr(ya), x.size, _ptr(out)), "roman_debug_math")
        return out

    def debug_cosine(self, params, D1, D2):
        D1, D2 = _f64(D1), _f64(D2)
        out = np.zeros((D1.shape[0], D2.shape[0]), dtype=np.float64)
        self._generation += 1
        self._check(self._lib.roman_debug_cosine(self._h, C.byref(params), _ptr(D1), D1.shape[0], _ptr(D2), D2.shape[0],
                                                 D1.shape[1], _ptr(out)), "roman_debug_cosine")
        return out


    def cosine_matrix(self, A, B):
        """Normalised cosine of every row of A (n1, d) with every row of B (n2, d) on the f64 matrix core (k_cos);
        0 where a row has zero norm.  Used for the submap-descriptor gate of the pair loop."""
        A, B = _f64(A), _f64(B)
        if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
            raise ValueError("cosine_matrix needs two (n, d) matrices of the same d")
        P = _abi.RomanParams.default()
        P.cos_feature_dim = A.shape[1]
        pad = lambda M: np.ascontiguousarray(np.hstack([np.zeros((M.shape[0], P.point_dim)), M]))     # [xyz | descriptor]
        if A.shape[0] == 0 or B.shape[0] == 0:
            return np.zeros((A.shape[0], B.shape[0]))
        return self.debug_cosine(P, pad(A), pad(B))


_DEFAULT_CTX = None


def default_context():
    """Process-wide context on HIP device 0 (created on first use; fails loudly without a GPU)."""
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = Context(0)
    return _DEFAULT_CTX


def version():
    return _abi.load_library().roman_version().decode()
