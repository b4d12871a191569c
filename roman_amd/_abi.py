"""ctypes mirror of include/roman_hip.h (structs + loader of libroman_hip.so).

The structs are shared with the test oracle (oracle/oracle.py) so both sides of a parity test
are driven by the same parameter block.  The library loader fails loudly: there is no Python /
CPU fallback behind the C ABI.
"""
import ctypes as C
import os

ROMAN_MAX_RATIO_FEATURES = 8

# error codes / status flags (include/roman_hip.h)
ROMAN_OK = 0
ROMAN_E_INVALID = -1
ROMAN_E_NOMEM = -4
ROMAN_E_UNSUPPORTED = -5
ROMAN_E_TOO_LARGE = -6
ROMAN_E_INTERNAL = -7
ROMAN_ST_OK = 0
ROMAN_ST_EMPTY_MAP = 1
ROMAN_ST_INSUFFICIENT = 2
ROMAN_ST_MAXITER = 4
ROMAN_ST_ASSOC_TRUNCATED = 8
ROMAN_ST_TIE_FALLBACK = 16
ROMAN_ST_WORKSPACE = 32
ROMAN_ST_INTERNAL = 64

ROMAN_INV_EUCLIDEAN = 0
ROMAN_INV_ROMAN = 1
ROMAN_INV_EUCLIDEAN_PRUNED = 2

ROMAN_FUSE_GEOMETRIC_MEAN = 0
ROMAN_FUSE_ARITHMETIC_MEAN = 1
ROMAN_FUSE_PRODUCT = 2

ROMAN_GRAV_COMBINED = 0
ROMAN_GRAV_SEPARATE = 1
ROMAN_GRAV_ZGATE = 2
ROMAN_SINGLE_BOTH = 0
ROMAN_SINGLE_OFFDIAG = 1
ROMAN_SINGLE_DIAG = 2
ROMAN_SINGLE_DIAG_KEEP = 3

ROMAN_STAGE_SINGLE = 0
ROMAN_STAGE_COUNT_PASS = 1
ROMAN_STAGE_FILL = 2
ROMAN_STAGE_SOLVE = 3
ROMAN_STAGE_COUNT = 4
STAGE_NAMES = ("single", "count", "fill", "solve")

# flag bits of roman_lc_record_t.flags
ROMAN_LC_ACCEPTED = 1
ROMAN_LC_FAILED_INSUFFICIENT = 2
ROMAN_LC_FAILED_TILT = 4
ROMAN_LC_FAILED_UPSIDE_DOWN = 8
ROMAN_LC_SKIPPED = 16
ROMAN_LC_INTERNAL = 32
ROMAN_LC_FAILED = ROMAN_LC_FAILED_INSUFFICIENT | ROMAN_LC_FAILED_TILT | ROMAN_LC_FAILED_UPSIDE_DOWN


class RomanParams(C.Structure):
    """roman_params_t"""
    _fields_ = [
        ("invariant", C.c_int32),
        ("point_dim", C.c_int32),
        ("ratio_feature_dim", C.c_int32),
        ("cos_feature_dim", C.c_int32),
        ("fusion_method", C.c_int32),
        ("gravity_guided", C.c_int32),
        ("drift_aware", C.c_int32),
        ("rescale_u0", C.c_int32),
        ("sigma", C.c_double),
        ("epsilon", C.c_double),
        ("mindist", C.c_double),
        ("distance_weight", C.c_double),
        ("ratio_weight", C.c_double),
        ("cosine_weight", C.c_double),
        ("cosine_min", C.c_double),
        ("cosine_max", C.c_double),
        ("gravity_unc_ang_rad", C.c_double),
        ("ratio_epsilon", C.c_double * ROMAN_MAX_RATIO_FEATURES),
        ("tol_u", C.c_double),
        ("tol_F", C.c_double),
        ("beta", C.c_double),
        ("eps", C.c_double),
        ("affinityeps", C.c_double),
        ("maxiniters", C.c_int32),
        ("maxoliters", C.c_int32),
        ("maxlsiters", C.c_int32),
        ("gravity_mode", C.c_int32),
        ("single_mode", C.c_int32),
        ("reserved", C.c_int32),
    ]

    @classmethod
    def default(cls):
        """Same values as roman_params_default() (kept in Python so parameter blocks can be
        built without a GPU; tests check the two agree)."""
        p = cls()
        p.invariant = ROMAN_INV_ROMAN
        p.point_dim = 3
        p.fusion_method = ROMAN_FUSE_GEOMETRIC_MEAN
        p.rescale_u0 = 1
        p.sigma, p.epsilon, p.mindist = 0.4, 0.6, 0.2
        p.distance_weight = p.ratio_weight = p.cosine_weight = 1.0
        p.cosine_min, p.cosine_max = 0.5, 0.7
        p.gravity_unc_ang_rad = 0.0872665
        p.tol_u, p.tol_F, p.beta, p.eps, p.affinityeps = 1e-8, 1e-9, 0.25, 1e-9, 1e-4
        p.maxiniters, p.maxoliters, p.maxlsiters = 200, 1000, 99
        return p

    def feature_dim(self):
        return self.point_dim + self.ratio_feature_dim + self.cos_feature_dim

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if name == "ratio_epsilon" else v
        return d


class RomanStats(C.Structure):
    """roman_stats_t"""
    _fields_ = [
        ("n_assoc_in", C.c_int32),
        ("n_live", C.c_int32),
        ("nnz_upper", C.c_int64),
        ("n_pass", C.c_int32),
        ("outer_iters", C.c_int32),
        ("inner_iters", C.c_int32),
        ("ls_trials", C.c_int32),
        ("score", C.c_double),
        ("d_final", C.c_double),
    ]


class RomanLcParams(C.Structure):
    """roman_lc_params_t"""
    _fields_ = [
        ("dim", C.c_int32),
        ("force_rm_upside_down", C.c_int32),
        ("force_rm_lc_roll_pitch", C.c_int32),
        ("lc_association_thresh", C.c_int32),
        ("tilt_thresh", C.c_double),
        ("reserved", C.c_int32 * 2),
    ]


class RomanLcRecord(C.Structure):
    """roman_lc_record_t"""
    _fields_ = [
        ("problem", C.c_int32),
        ("n_assoc", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
        ("T_hat", C.c_double * 16),
        ("theta", C.c_double),
        ("dist", C.c_double),
        ("edge_t", C.c_double * 3),
        ("edge_q", C.c_double * 4),
    ]


class RomanMnoSolution(C.Structure):
    """roman_mno_solution_t"""
    _fields_ = [
        ("n_assoc", C.c_int32),
        ("status", C.c_int32),
        ("score", C.c_double),
        ("T", C.c_double * 16),
    ]


ROMAN_MNO_MAX_SOLUTIONS = 64
ROMAN_MNO_MAX_ASSOC = 3072


class RomanRansacParams(C.Structure):
    """roman_ransac_params_t"""
    _fields_ = [
        ("max_iteration", C.c_int64),
        ("round", C.c_int32),
        ("edge_len", C.c_double),
        ("max_dist", C.c_double),
        ("confidence", C.c_double),
        ("seed", C.c_uint64),
    ]


class RomanRansacRecord(C.Structure):
    """roman_ransac_record_t"""
    _fields_ = [
        ("n_assoc", C.c_int32),
        ("status", C.c_int32),
        ("n_hyp", C.c_int64),
        ("n_scored", C.c_int64),
        ("best_hyp", C.c_int64),
        ("best_count", C.c_int32),
        ("best_sse", C.c_double),
        ("T", C.c_double * 16),
    ]


ROMAN_RANSAC_MAX_OBJECTS = 1024


class RomanSubmapParams(C.Structure):
    """roman_submap_params_t"""
    _fields_ = [
        ("point_dim", C.c_int32),
        ("max_size", C.c_int32),
        ("cap", C.c_int32),
        ("prune_by_time", C.c_int32),
        ("use_radius", C.c_int32),
        ("reserved0", C.c_int32),
        ("radius", C.c_double),
        ("reserved", C.c_int32 * 2),
    ]


class RomanSubmapDesc(C.Structure):
    """roman_submap_desc_t"""
    _fields_ = [
        ("pos", C.c_double * 3),
        ("T_center_odom", C.c_double * 16),
        ("time", C.c_double),
        ("t_hi", C.c_double),
        ("t_lo", C.c_double),
    ]


class RomanGridGateParams(C.Structure):
    """roman_grid_gate_params_t"""
    _fields_ = [
        ("radius", C.c_double),
        ("skip_distance", C.c_double),
        ("desc_dim", C.c_int32),
        ("reserved0", C.c_int32),
        ("desc_thresh", C.c_double),
        ("single_robot_lc", C.c_int32),
        ("reserved1", C.c_int32),
        ("lc_time_thresh", C.c_double),
        ("reserved", C.c_int32 * 2),
    ]


class RomanFrameSelectParams(C.Structure):
    """roman_frame_select_params_t"""
    _fields_ = [
        ("thin", C.c_int32),
        ("want_mean", C.c_int32),
        ("thin_dist", C.c_double),
        ("reserved", C.c_int32 * 2),
    ]


class RomanSessionFrameRobot(C.Structure):
    """roman_session_frame_robot_t"""
    _fields_ = [
        ("seg0", C.c_int64),
        ("mask_off", C.c_int64),
        ("n_seg", C.c_int32),
        ("sub0", C.c_int32),
        ("n_sub", C.c_int32),
        ("frame0", C.c_int32),
        ("n_frames", C.c_int32),
        ("mask_words", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class RomanSegmentShapeParams(C.Structure):
    """roman_segment_shape_params_t"""
    _fields_ = [
        ("center_ref", C.c_int32),
        ("out_stride", C.c_int32),
        ("col_center", C.c_int32),
        ("col_pca", C.c_int32),
        ("col_volume", C.c_int32),
        ("col_extent", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


ROMAN_CENTER_MEAN = 0
ROMAN_CENTER_BOTTOM_MIDDLE = 1
CENTER_REFS = {"mean": ROMAN_CENTER_MEAN, "bottom_middle": ROMAN_CENTER_BOTTOM_MIDDLE}     # the strings of [REF roman/object/segment.py:266-274]
# flag bits of roman_segment_shapes' status[]
ROMAN_SEG_EMPTY = 1
ROMAN_SEG_FEW_POINTS = 2
ROMAN_SEG_DEGENERATE = 4
ROMAN_SEG_BLOCK_MIN = 768   # points from which a segment takes a workgroup instead of a wave (kernels.hip.h SEG_BLOCK_MIN)


class RomanAssocParams(C.Structure):
    """roman_assoc_params_t"""
    _fields_ = [
        ("voxel_size", C.c_double),
        ("geometric", C.c_int32),
        ("semantic", C.c_int32),
        ("geo_range", C.c_double * 2),
        ("sem_range", C.c_double * 2),
    ]


ROMAN_ASSOC_IOU = 0
ROMAN_ASSOC_IOM = 1
ASSOC_GEOMETRIC = {"iou": ROMAN_ASSOC_IOU, "iom": ROMAN_ASSOC_IOM}     # geometric_association_method [REF roman/map/mapper.py:150-154] without 'chamfer'
# roman_assoc_scores' status[]
ROMAN_ASSOC_OK = 0
ROMAN_ASSOC_EMPTY = 1
ROMAN_ASSOC_RANGE = 2
ROMAN_ASSOC_WAVE_MAX = 256  # points up to which one wave sorts a cloud's keys (kernels.hip.h ASSOC_WAVE_MAX)
ROMAN_ASSOC_LDS_MAX = 8192  # ... up to which a workgroup sorts them in LDS alone (kernels.hip.h ASSOC_LDS_MAX)
ASSOC_PARAMS_NBYTES = C.sizeof(RomanAssocParams)


class RomanIntegrateParams(C.Structure):
    """roman_integrate_params_t"""
    _fields_ = [
        ("voxel_size", C.c_double),
        ("outlier_std", C.c_double),
        ("nb_neighbors", C.c_int32),
    ]


class RomanIntegrateJob(C.Structure):
    """roman_integrate_job_t"""
    _fields_ = [("base", C.c_int32), ("add", C.c_int32), ("pose", C.c_int32)]


ROMAN_INTEGRATE_NEIGHBORS = 10      # nb_neighbors of remove_statistical_outlier [REF roman/object/segment.py:183-184]; the only value served
ROMAN_INTEGRATE_WAVE_MAX = 256      # points (base + added) up to which one wave takes a job (kernels.hip.h INTEG_WAVE_MAX)
ROMAN_INTEGRATE_LDS_MAX = 4096      # ... up to which a workgroup sorts the job in LDS alone (kernels.hip.h INTEG_LDS_CAP)
INTEGRATE_PARAMS_NBYTES = C.sizeof(RomanIntegrateParams)
INTEGRATE_JOB_DTYPE = [("base", "<i4"), ("add", "<i4"), ("pose", "<i4")]      # roman_integrate_job_t as a structured dtype


class RomanClusterParams(C.Structure):
    """roman_cluster_params_t"""
    _fields_ = [("eps", C.c_double), ("min_points", C.c_int32)]


ROMAN_CLUSTER_MIN_POINTS = 10       # final_cleanup's default min_points [REF roman/object/segment.py:195]
ROMAN_CLUSTER_WAVE_MAX = 256        # points up to which one wave takes a job (kernels.hip.h CLUS_WAVE_MAX)
ROMAN_CLUSTER_LDS_MAX = 1536        # ... up to which a workgroup holds the job in LDS (kernels.hip.h CLUS_LDS_CAP)
ROMAN_CLUSTER_TILE = 256            # query points of one workgroup of the tiled class (kernels.hip.h CLUS_TILE)
ROMAN_CLUSTER_COLS = 1024           # column points the tiled class stages at a time (kernels.hip.h CLUS_COLS)
CLUSTER_PARAMS_NBYTES = C.sizeof(RomanClusterParams)

# flag bits of roman_grid_gate's flags[]
ROMAN_GRID_NEARBY = 1
ROMAN_GRID_SKIP = 2
ROMAN_GRID_GATED = 4
ROMAN_GRID_TODO = 8

GRID_TJ = 4                 # columns of a row one wave of the gate kernels takes (kernels.hip.h): the unit of roman_session_gate's tile_off
SESSION_SCAN = 1024         # flags per workgroup of roman_session_gate's compaction (kernels.hip.h)

SUBMAP_LDS_CAND = 4096      # candidates of a submap the select kernel holds in LDS (kernels.hip.h); more go through the context's scratch

STATS_NBYTES = C.sizeof(RomanStats)
MNO_SOLUTION_NBYTES = C.sizeof(RomanMnoSolution)
RANSAC_RECORD_NBYTES = C.sizeof(RomanRansacRecord)
SUBMAP_PARAMS_NBYTES = C.sizeof(RomanSubmapParams)
SUBMAP_DESC_NBYTES = C.sizeof(RomanSubmapDesc)
GRID_GATE_PARAMS_NBYTES = C.sizeof(RomanGridGateParams)
FRAME_SELECT_PARAMS_NBYTES = C.sizeof(RomanFrameSelectParams)
SESSION_FRAME_ROBOT_NBYTES = C.sizeof(RomanSessionFrameRobot)
SEGMENT_SHAPE_PARAMS_NBYTES = C.sizeof(RomanSegmentShapeParams)
STACKED_BAND_MIN = 32       # the smallest row band of roman_stacked_sim* (kernels.hip.h STACK_TILE)
LC_PARAMS_NBYTES = C.sizeof(RomanLcParams)
LC_RECORD_NBYTES = C.sizeof(RomanLcRecord)
PARAMS_NBYTES = C.sizeof(RomanParams)

_LIB = None
# in-tree build product (roman_amd/csrc/Makefile); ROMAN_HIP_LIBRARY overrides the location
_LIB_PATH = os.environ.get("ROMAN_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libroman_hip.so")


class RomanHipError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def load_library():
    """dlopen libroman_hip.so and declare the prototypes of every symbol in roman_hip.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise RomanHipError(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for roman_amd.")
    lib = C.CDLL(_LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    P = C.POINTER
    ctxp = vp
    protos = {
        "roman_params_default": (C.c_int, [P(RomanParams)]),
        "roman_ctx_create": (C.c_int, [P(ctxp), C.c_int, vp]),
        "roman_ctx_destroy": (C.c_int, [ctxp]),
        "roman_ctx_set_pipeline": (C.c_int, [ctxp, C.c_int]),
        "roman_ctx_sync": (C.c_int, [ctxp]),
        "roman_ctx_set_host_batching": (C.c_int, [ctxp, C.c_int, C.c_int]),
        "roman_ctx_set_wide_teams": (C.c_int, [ctxp, C.c_int]),
        "roman_ctx_join": (C.c_int, [ctxp, C.c_int]),
        "roman_ctx_join_on": (C.c_int, [ctxp, C.c_int, C.c_void_p]),
        "roman_ctx_skipped": (C.c_int, [ctxp, C.c_int, P(i64)]),
        "roman_last_error": (C.c_char_p, [ctxp]),
        "roman_align_batch_dev": (C.c_int, [ctxp, P(RomanParams), i32, vp, vp, vp, vp, vp, i32,
                                            vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_align_batch": (C.c_int, [ctxp, P(RomanParams), i32, vp, i64, vp, vp, vp, vp, i32,
                                        vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_align_batch_resident": (C.c_int, [ctxp, P(RomanParams), i32, vp, vp, vp, vp, vp, i32,
                                                 vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_lc_tail_dev": (C.c_int, [ctxp, P(RomanLcParams), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "roman_align_lc_batch_dev": (C.c_int, [ctxp, P(RomanParams), i32, vp, vp, vp, vp, vp, i32,
                                               vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                               P(RomanLcParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "roman_align_lc_batch": (C.c_int, [ctxp, P(RomanParams), i32, vp, i64, vp, vp, vp, vp, i32,
                                           vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                           P(RomanLcParams), vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
        "roman_shared_ids_dev": (C.c_int, [ctxp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "roman_shared_reduce_dev": (C.c_int, [ctxp, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "roman_align_lc_batch_ids": (C.c_int, [ctxp, P(RomanParams), i32, vp, i64, vp, vp, vp, vp, i32,
                                               vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                               P(RomanLcParams), vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp,
                                               vp, vp, vp, vp]),
        "roman_mno_batch_dev": (C.c_int, [ctxp, P(RomanParams), i32, vp, vp, vp, vp, vp, i32,
                                          vp, vp, i32, i32, vp, vp, vp]),
        "roman_mno_batch": (C.c_int, [ctxp, P(RomanParams), i32, vp, i64, vp, vp, vp, vp, i32,
                                      vp, vp, i32, i32, vp, vp, vp]),
        "roman_mno_lc_tail_dev": (C.c_int, [ctxp, P(RomanLcParams), i32, i32] + [vp] * 13),
        "roman_mno_lc_batch_dev": (C.c_int, [ctxp, P(RomanParams), i32, vp, vp, vp, vp, vp, i32,
                                             vp, vp, i32, i32, vp, vp, vp,
                                             P(RomanLcParams)] + [vp] * 12),
        "roman_mno_lc_batch": (C.c_int, [ctxp, P(RomanParams), i32, vp, i64, vp, vp, vp, vp, i32,
                                         vp, vp, i32, i32, vp, vp, vp,
                                         P(RomanLcParams), vp, vp, vp, i32, vp, vp, i32, vp] + [vp] * 6),
        "roman_ransac_batch_dev": (C.c_int, [ctxp, P(RomanRansacParams), i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
        "roman_ransac_batch": (C.c_int, [ctxp, P(RomanRansacParams), i32, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]),
        "roman_ransac_lc_batch_dev": (C.c_int, [ctxp, P(RomanRansacParams), i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                                P(RomanLcParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "roman_ransac_lc_batch": (C.c_int, [ctxp, P(RomanRansacParams), i32, vp, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                            P(RomanLcParams), vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
        "roman_submaps_dev": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
        "roman_submaps": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
        "roman_session_submaps_dev": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32] + [vp] * 11 + [i32, vp]),
        "roman_session_submaps": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32] + [vp] * 11 + [i32, vp]),
        "roman_session_submaps_list_dev": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32] + [vp] * 11 + [i32, vp, i32, vp, vp]),
        "roman_session_submaps_list": (C.c_int, [ctxp, P(RomanSubmapParams), i32, i32] + [vp] * 11 + [i32, vp, i32, vp, vp]),
        "roman_grid_gate_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 19),
        "roman_grid_gate": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 19),
        "roman_grid_gate_sim_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 17),
        "roman_grid_gate_sim": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 17),
        "roman_submaps_fill_dev": (C.c_int, [ctxp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp]),
        "roman_submaps_fill": (C.c_int, [ctxp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp]),
        "roman_submap_boxes_dev": (C.c_int, [ctxp, i32, i32, i32, vp, vp, vp, vp]),
        "roman_submap_boxes": (C.c_int, [ctxp, i32, i32, i32, vp, vp, vp, vp]),
        "roman_grid_gate_aabb_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 22),
        "roman_grid_gate_aabb": (C.c_int, [ctxp, P(RomanGridGateParams), i32, i32] + [vp] * 22),
        "roman_session_gate_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 8 + [i32] + [vp] * 15),
        "roman_session_gate": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 7 + [i32] + [vp] * 12),
        "roman_session_gate_sim_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 8 + [i32] + [vp] * 16),
        "roman_session_gate_sim": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 7 + [i32] + [vp] * 13),
        "roman_session_stacked_sim_dev": (C.c_int, [ctxp, i32, i32, vp, vp, i32] + [vp] * 8 + [i32] + [vp] * 5),
        "roman_session_stacked_sim": (C.c_int, [ctxp, i32, i32, vp, vp, i64, i32] + [vp] * 4 + [i32] + [vp] * 3),
        "roman_session_stacked_sim_list_dev": (C.c_int, [ctxp, i32, i32, vp, vp, i32] + [vp] * 8 + [i32] + [vp] * 4 + [i32] + [vp] * 3),
        "roman_session_stacked_sim_list": (C.c_int, [ctxp, i32, i32, vp, vp, i64, i32] + [vp] * 4 + [i32] + [vp] * 2 + [i32] + [vp] * 2),
        "roman_session_boxes_dev": (C.c_int, [ctxp, i32, i32, vp, vp, vp, vp, vp]),
        "roman_session_boxes": (C.c_int, [ctxp, i32, i32, vp, vp, vp, vp, vp]),
        "roman_session_gate_aabb_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 8 + [i32] + [vp] * 17),
        "roman_session_gate_aabb": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 7 + [i32] + [vp] * 14),
        "roman_session_gate_list_dev": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 8 + [i32] + [vp] * 4 + [i32] + [vp] * 13),
        "roman_session_gate_list": (C.c_int, [ctxp, P(RomanGridGateParams), i32] + [vp] * 7 + [i32] + [vp] * 2 + [i32] + [vp] * 12),
        "roman_frame_select_dev": (C.c_int, [ctxp, P(RomanFrameSelectParams), i32, i32, vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_frame_select": (C.c_int, [ctxp, P(RomanFrameSelectParams), i32, i32, vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_session_frame_select_list_dev": (C.c_int, [ctxp, P(RomanFrameSelectParams), i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32] + [vp] * 6),
        "roman_session_frame_select_list": (C.c_int, [ctxp, P(RomanFrameSelectParams), i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32] + [vp] * 6),
        "roman_stacked_sim_dev": (C.c_int, [ctxp, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp]),
        "roman_stacked_sim": (C.c_int, [ctxp, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp]),
        "roman_ctx_set_stacked_band": (C.c_int, [ctxp, i32]),
        "roman_segment_shapes_dev": (C.c_int, [ctxp, vp, vp, vp, i32, P(RomanSegmentShapeParams), vp, vp]),
        "roman_segment_shapes": (C.c_int, [ctxp, vp, vp, i32, P(RomanSegmentShapeParams), vp, vp]),
        "roman_ctx_set_segment_block_min": (C.c_int, [ctxp, i32]),
        "roman_assoc_scores_dev": (C.c_int, [ctxp, P(RomanAssocParams), vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "roman_assoc_scores": (C.c_int, [ctxp, P(RomanAssocParams), vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "roman_ctx_set_assoc_cuts": (C.c_int, [ctxp, i32, i32]),
        "roman_segment_integrate_dev": (C.c_int, [ctxp, P(RomanIntegrateParams), vp, vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "roman_segment_integrate": (C.c_int, [ctxp, P(RomanIntegrateParams), vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "roman_ctx_set_integrate_cuts": (C.c_int, [ctxp, i32, i32]),
        "roman_segment_cluster_dev": (C.c_int, [ctxp, P(RomanClusterParams), vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "roman_segment_cluster": (C.c_int, [ctxp, P(RomanClusterParams), vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "roman_ctx_set_cluster_cuts": (C.c_int, [ctxp, i32, i32]),
        "roman_ctx_has_history": (C.c_int, [ctxp, P(RomanParams), i32, P(i32)]),
        "roman_ctx_cosine_screen_stats": (C.c_int, [ctxp, P(C.c_int64), P(C.c_int64), P(C.c_double)]),
        "roman_create_all_to_all": (C.c_int, [i32, i32, vp]),
        "roman_deal_problems": (C.c_int, [i32, vp, vp, vp, i32, i32, vp, P(i32)]),
        "roman_score": (C.c_int, [ctxp, P(RomanParams), vp, i32, vp, i32, i32, vp, i32]),
        "roman_set_matrix_data": (C.c_int, [ctxp, P(RomanParams), vp, vp, i32]),
        "roman_solve": (C.c_int, [ctxp, vp]),
        "roman_num_associations": (C.c_int, [ctxp, P(i32)]),
        "roman_num_selected": (C.c_int, [ctxp, P(i32)]),
        "roman_get_selected_associations": (C.c_int, [ctxp, vp]),
        "roman_get_solution": (C.c_int, [ctxp, vp, vp, P(dbl), P(RomanStats)]),
        "roman_get_dense_matrices": (C.c_int, [ctxp, vp, vp]),
        "roman_get_upper_csr": (C.c_int, [ctxp, P(i64), vp, vp, vp, vp]),
        "roman_pose_batch": (C.c_int, [ctxp, i32, i32, vp, vp, vp, vp, vp]),
        "roman_profile_enable": (C.c_int, [ctxp, C.c_int]),
        "roman_profile_reset": (C.c_int, [ctxp]),
        "roman_profile_get": (C.c_int, [ctxp, P(dbl), P(i64)]),
        "roman_debug_math": (C.c_int, [ctxp, C.c_int, vp, vp, i64, vp]),
        "roman_debug_cosine": (C.c_int, [ctxp, P(RomanParams), vp, i32, vp, i32, i32, vp]),
        "roman_debug_live": (C.c_int, [ctxp, P(i32), vp, vp]),
        "roman_version": (C.c_char_p, []),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)          # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    lib._roman_symbols = tuple(protos)
    _LIB = lib
    return lib


EXPORTED_SYMBOLS = (
    "roman_params_default", "roman_ctx_create", "roman_ctx_destroy", "roman_ctx_set_pipeline", "roman_ctx_sync", "roman_ctx_set_host_batching", "roman_ctx_set_wide_teams", "roman_ctx_join", "roman_ctx_join_on",
    "roman_ctx_skipped", "roman_last_error",
    "roman_align_batch_dev", "roman_align_batch", "roman_align_batch_resident", "roman_lc_tail_dev", "roman_align_lc_batch_dev", "roman_align_lc_batch", "roman_shared_ids_dev", "roman_shared_reduce_dev", "roman_align_lc_batch_ids", "roman_mno_batch_dev", "roman_mno_batch", "roman_mno_lc_tail_dev", "roman_mno_lc_batch_dev", "roman_mno_lc_batch", "roman_ransac_batch_dev", "roman_ransac_batch", "roman_ransac_lc_batch_dev", "roman_ransac_lc_batch", "roman_submaps_dev", "roman_submaps", "roman_session_submaps_dev", "roman_session_submaps", "roman_session_submaps_list_dev", "roman_session_submaps_list", "roman_grid_gate_dev", "roman_grid_gate", "roman_grid_gate_sim_dev", "roman_grid_gate_sim", "roman_submaps_fill_dev", "roman_submaps_fill", "roman_submap_boxes_dev", "roman_submap_boxes", "roman_grid_gate_aabb_dev", "roman_grid_gate_aabb", "roman_session_gate_dev", "roman_session_gate", "roman_session_gate_sim_dev", "roman_session_gate_sim", "roman_session_stacked_sim_dev", "roman_session_stacked_sim", "roman_session_stacked_sim_list_dev", "roman_session_stacked_sim_list", "roman_session_boxes_dev", "roman_session_boxes", "roman_session_gate_aabb_dev", "roman_session_gate_aabb", "roman_session_gate_list_dev", "roman_session_gate_list", "roman_frame_select_dev", "roman_frame_select", "roman_session_frame_select_list_dev", "roman_session_frame_select_list", "roman_stacked_sim_dev", "roman_stacked_sim", "roman_ctx_set_stacked_band", "roman_segment_shapes_dev", "roman_segment_shapes", "roman_ctx_set_segment_block_min", "roman_assoc_scores_dev", "roman_assoc_scores", "roman_ctx_set_assoc_cuts", "roman_segment_integrate_dev", "roman_segment_integrate", "roman_ctx_set_integrate_cuts", "roman_segment_cluster_dev", "roman_segment_cluster", "roman_ctx_set_cluster_cuts", "roman_ctx_has_history", "roman_ctx_cosine_screen_stats", "roman_deal_problems", "roman_create_all_to_all", "roman_score",
    "roman_set_matrix_data", "roman_solve", "roman_num_associations", "roman_num_selected",
    "roman_get_selected_associations", "roman_get_solution", "roman_get_dense_matrices",
    "roman_get_upper_csr", "roman_pose_batch", "roman_profile_enable", "roman_profile_reset",
    "roman_profile_get", "roman_debug_math", "roman_debug_cosine", "roman_debug_live",
    "roman_version",
)
