"""The loop-closure tail stated in vectorised NumPy (no scipy objects per pair), the cases that exercise it and the
EXISTING per-pair code run on those cases.

`lc_tail()` is the CPU double behind `submap_align_grid(compute=...)` and the expectation of the GPU tests for
`roman_lc_tail_dev` / `roman_align_lc_batch`: the arithmetic of `submap_align()` pass 2 + `loop_closure_edges()` +
`transform_to_xyz_quat()` (roman_amd/align/submap_align.py), batch-wide.

`make_cases()` plants the situations the tail has to decide: rotations beside gimbal lock, roll / pitch on both sides of 90
degrees and of the 5 degree tilt threshold, every failure status with its NaN pose, association counts at
thresh - 1 / thresh / thresh + 1, a pair the time gate disables.  Every planted angle keeps at least MARGIN from a
threshold (a decision AT a threshold depends on atan2's last bits, which differ between libraries); reflections never
occur (T_align rejects them upstream: every planted rotation is checked to have determinant +1).
`per_pair_reference()` runs the existing functions on the same cases.
"""
import numpy as np

from roman_amd import _abi
from roman_amd.align import submap_align as sa
from roman_amd.runtime import BatchResult, LcInputs, LoopClosureResult, lc_record_dtype, stats_dtype

MARGIN = 1e-6                      # radians every planted angle keeps from 90 degrees and from the tilt threshold
TILT = float(np.deg2rad(5))        # DistRegWithPruning's default roll_pitch_thresh
THRESH = 4                         # lc_association_thresh of the cases


# ---------------------------------------------------------------------------------------------
# the tail in NumPy
# ---------------------------------------------------------------------------------------------
def quat_from_matrix(R):
    """(K,3,3) -> (K,4) xyzw with the branch rule of scipy's Rotation.from_matrix: the first maximum of
    (R00, R11, R22, trace) picks the component computed as a sum; normalised, not canonicalised."""
    K = R.shape[0]
    dec = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], axis=1)
    choice = np.argmax(dec, axis=1) if K else np.zeros(0, dtype=np.int64)
    q = np.empty((K, 4))
    for i in range(3):
        m = choice == i
        j = (i + 1) % 3; k = (j + 1) % 3
        q[m, i] = 1 - dec[m, 3] + 2 * R[m, i, i]
        q[m, j] = R[m, j, i] + R[m, i, j]
        q[m, k] = R[m, k, i] + R[m, i, k]
        q[m, 3] = R[m, k, j] - R[m, j, k]
    m = choice == 3
    q[m, 0] = R[m, 2, 1] - R[m, 1, 2]; q[m, 1] = R[m, 0, 2] - R[m, 2, 0]; q[m, 2] = R[m, 1, 0] - R[m, 0, 1]; q[m, 3] = 1 + dec[m, 3]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def lc_tail(lc: LcInputs, T, n_assoc, status):
    """-> (records (B,) lc_record_dtype, accepted (K,) int32 ascending).  T: (B, dim+1, dim+1)."""
    status = np.asarray(status, dtype=np.int32); B = status.shape[0]
    n_assoc = np.asarray(n_assoc, dtype=np.int32)
    dim = int(lc.dim)
    T = np.asarray(T, dtype=np.float64).reshape(B, dim + 1, dim + 1)
    flags = np.zeros(B, dtype=np.int32)
    skipped = (status & _abi.ROMAN_ST_WORKSPACE) != 0
    internal = ~skipped & ((status & _abi.ROMAN_ST_INTERNAL) != 0)
    insufficient = ~skipped & ~internal & ((status & (_abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_EMPTY_MAP)) != 0)
    flags[skipped] = _abi.ROMAN_LC_SKIPPED; flags[internal] = _abi.ROMAN_LC_INTERNAL; flags[insufficient] = _abi.ROMAN_LC_FAILED_INSUFFICIENT
    ok = flags == 0
    Th = np.tile(np.eye(4), (B, 1, 1))
    if dim == 2:
        Th[:, :2, :2] = T[:, :2, :2]; Th[:, :2, 3] = T[:, :2, 2]
    else:
        Th[:] = T
        with np.errstate(invalid="ignore"):
            pitch = -np.arcsin(np.clip(Th[:, 2, 0], -1.0, 1.0))
            roll = np.arctan2(Th[:, 2, 1], Th[:, 2, 2])
            if lc.tilt_thresh is not None and lc.tilt_thresh >= 0:
                bad = ok & ~((np.abs(roll) < lc.tilt_thresh) & (np.abs(pitch) < lc.tilt_thresh))
                flags[bad] = _abi.ROMAN_LC_FAILED_TILT; ok &= ~bad
            if lc.force_rm_upside_down:
                bad = ok & ((np.abs(roll) > np.deg2rad(90.)) | (np.abs(pitch) > np.deg2rad(90.)))
                flags[bad] = _abi.ROMAN_LC_FAILED_UPSIDE_DOWN; ok &= ~bad
            if lc.force_rm_lc_roll_pitch:
                yaw = np.arctan2(Th[:, 1, 0], Th[:, 0, 0])
                Rz = np.zeros((B, 3, 3)); Rz[:, 2, 2] = 1.0
                Rz[:, 0, 0] = np.cos(yaw); Rz[:, 0, 1] = -np.sin(yaw); Rz[:, 1, 0] = np.sin(yaw); Rz[:, 1, 1] = np.cos(yaw)
                Th[ok, :3, :3] = Rz[ok]
    Th[~ok] = np.nan
    theta = np.full(B, 180.0); dist = np.full(B, 1e6)
    theta[ok] = np.nan; dist[ok] = np.nan
    if lc.T_ref is not None and np.any(ok):
        E = np.linalg.inv(Th[ok]) @ np.asarray(lc.T_ref, dtype=np.float64).reshape(B, 4, 4)[ok]
        if dim == 2:
            theta[ok] = np.arctan2(E[:, 1, 0], E[:, 0, 0]); dist[ok] = np.linalg.norm(E[:, :2, 3], axis=1)
        else:
            skew = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)
            theta[ok] = np.arctan2(0.5 * np.linalg.norm(skew, axis=1), 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0))
            dist[ok] = np.linalg.norm(E[:, :3, 3], axis=1)
    n = np.where(ok, n_assoc, 0).astype(np.int32)
    accepted = ~(skipped | internal) & (n >= lc.lc_association_thresh)
    if lc.enable is not None:
        accepted &= np.asarray(lc.enable).reshape(B) != 0
    flags[accepted] |= _abi.ROMAN_LC_ACCEPTED
    rec = np.zeros(B, dtype=lc_record_dtype())
    rec["problem"] = np.arange(B); rec["n_assoc"] = n; rec["flags"] = flags
    rec["T_hat"] = Th; rec["theta"] = theta; rec["dist"] = dist
    rec["edge_t"] = np.nan; rec["edge_q"] = np.nan
    acc = np.nonzero(accepted)[0].astype(np.int32)
    if acc.size:
        E = Th[acc]
        if lc.FL is not None:
            E = np.asarray(lc.FL, dtype=np.float64).reshape(-1, 4, 4)[np.asarray(lc.iL)[acc]] @ E
        if lc.FR is not None:
            E = E @ np.asarray(lc.FR, dtype=np.float64).reshape(-1, 4, 4)[np.asarray(lc.iR)[acc]]
        rec["edge_t"][acc] = E[:, :3, 3]
        with np.errstate(invalid="ignore"):
            rec["edge_q"][acc] = quat_from_matrix(E[:, :3, :3])
    return rec, acc


def as_lc_result(batch_result, lc):
    """A BatchResult + the NumPy tail -> what align_lc_batch returns."""
    n = np.array([len(a) for a in batch_result.assoc], dtype=np.int32)
    rec, acc = lc_tail(lc, batch_result.T, n, batch_result.status)
    return LoopClosureResult(batch_result.assoc, batch_result.T, batch_result.status, batch_result.stats, rec, acc)


def oracle_lc_compute(registration, batch, lc):
    """CPU double for run_lc_batch: the oracle per problem (tests/test_submap_align.py's double), then the NumPy tail."""
    from test_submap_align import oracle_compute
    return as_lc_result(oracle_compute(registration, batch), lc)


# ---------------------------------------------------------------------------------------------
# comparisons (tolerances of tests/test_submap_align.py for the same quantities)
# ---------------------------------------------------------------------------------------------
def assert_records_match(got, got_acc, want, want_acc, abs_theta=False):
    """Flags, counts and the accepted list identical; floats within 1e-8 (poses, edges), 1e-7 (dist), 1e-5 (angle in degrees).
    Quaternions as given, not up to sign.  abs_theta: `want` comes from submap_align(), which keeps |theta| only."""
    if abs_theta:
        got = got.copy(); got["theta"] = np.abs(got["theta"])
    assert got.shape == want.shape
    np.testing.assert_array_equal(got["flags"], want["flags"])
    np.testing.assert_array_equal(got["n_assoc"], want["n_assoc"])
    np.testing.assert_array_equal(got["problem"], want["problem"])
    np.testing.assert_array_equal(np.asarray(got_acc), np.asarray(want_acc))
    np.testing.assert_allclose(got["T_hat"], want["T_hat"], rtol=0, atol=1e-8, equal_nan=True)
    np.testing.assert_allclose(got["dist"], want["dist"], rtol=0, atol=1e-7, equal_nan=True)
    np.testing.assert_allclose(np.rad2deg(got["theta"]), np.rad2deg(want["theta"]), rtol=0, atol=1e-5, equal_nan=True)
    np.testing.assert_allclose(got["edge_t"], want["edge_t"], rtol=0, atol=1e-8, equal_nan=True)
    np.testing.assert_allclose(got["edge_q"], want["edge_q"], rtol=0, atol=1e-8, equal_nan=True)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def sa_rot(yaw, pitch, roll):
    from roman_amd.synth import yaw_transform
    return yaw_transform(yaw, [0, 0, 0], roll=roll, pitch=pitch)[:3, :3]


class _Seg:
    def __init__(self, id):
        self.id = id
        self.center = np.zeros((3, 1))


class FrameSubmap(sa.Submap):
    """A submap whose gravity-aligned pose is a COPY (what a caller's own map class may do): loop_closure_edges() then
    composes non-trivial frames around the estimate, which the in-place stand-in reduces to inv(X) @ X."""

    @property
    def pose_gravity_aligned(self):
        return sa.transform_rm_roll_pitch(self.pose_flu.copy())


class StubRegistration:
    """Just enough of a registration object for submap_align() with an injected compute."""

    def __init__(self, dim, use_gravity):
        self.dim = dim; self.use_gravity = use_gravity; self.roll_pitch_thresh = TILT

    def pack(self, segs):
        return np.zeros((len(segs), self.dim))

    def _association_list(self, a, b):
        return None

    def _abi_params(self):
        p = _abi.RomanParams.default(); p.invariant = _abi.ROMAN_INV_EUCLIDEAN; p.point_dim = self.dim
        return p


def make_cases(dim=3, seed=0, tilt=False, upside_down=True, rm_roll_pitch=True, S0=4, in_place=False):
    """-> dict: the planted batch (T, n_assoc, status), the submaps of an S0 x S1 grid whose pairs are the problems in
    row-major order, and the switches.  `tilt`: the pruning plugin's tilt check is on."""
    rng = np.random.default_rng(seed)
    h = np.pi / 2
    rots = []                                            # (yaw, pitch, roll)
    if dim == 3:
        for _ in range(12):                              # random attitudes of every size
            rots.append((rng.uniform(-np.pi, np.pi), rng.uniform(-h + 0.05, h - 0.05), rng.uniform(-np.pi, np.pi)))
        for _ in range(6):                               # small tilts, as estimates of gravity-aligned submaps are
            rots.append((rng.uniform(-np.pi, np.pi), rng.normal(0, 0.02), rng.normal(0, 0.02)))
        for s in (-1, 1):                                # beside gimbal lock (pitch within a milliradian of +-90 degrees)
            rots.append((0.3, s * (h - 1e-3), 0.2)); rots.append((-2.0, s * (h - 2e-3), -0.4))
        for s in (-1, 1):                                # roll on both sides of 90 degrees, as close as MARGIN allows
            for d in (-MARGIN, MARGIN, -1e-3, 1e-3):
                rots.append((rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.3), s * (h + d)))
        for s in (-1, 1):                                # roll / pitch on both sides of the tilt threshold
            for d in (-MARGIN, MARGIN, -1e-3, 1e-3):
                rots.append((rng.uniform(-np.pi, np.pi), 0.01, s * (TILT + d)))
                rots.append((rng.uniform(-np.pi, np.pi), s * (TILT + d), -0.01))
        rots.append((np.pi - 1e-9, 0.0, 0.0)); rots.append((0.0, 0.0, np.pi - 1e-3)); rots.append((0.0, 0.0, 0.0))
    else:
        for _ in range(20):
            rots.append((rng.uniform(-np.pi, np.pi), 0.0, 0.0))
    S1 = -(-(len(rots) + 12) // S0)
    B = S0 * S1
    while len(rots) < B:
        rots.append((rng.uniform(-np.pi, np.pi), rng.normal(0, 0.02) if dim == 3 else 0.0, rng.normal(0, 0.02) if dim == 3 else 0.0))
    T = np.zeros((B, dim + 1, dim + 1)); T[:, dim, dim] = 1.0
    for b, (y, p, r) in enumerate(rots):
        R = sa_rot(y, p, r)
        assert np.linalg.det(R) > 0.999                  # no reflections: T_align rejects them upstream
        T[b, :dim, :dim] = R[:dim, :dim]
        T[b, :dim, dim] = rng.uniform(-8, 8, dim)
    status = np.zeros(B, dtype=np.int32)
    n_assoc = rng.integers(THRESH + 2, 30, B).astype(np.int32)
    tail = B - 12                                        # the padded (benign: small tilt) cases carry the statuses and the counts
    n_assoc[tail + 6:tail + 9] = (THRESH - 1, THRESH, THRESH + 1)    # the acceptance threshold from both sides
    for k, st in enumerate((_abi.ROMAN_ST_INSUFFICIENT, _abi.ROMAN_ST_EMPTY_MAP, _abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_EMPTY_MAP,
                            _abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_MAXITER)):
        status[tail + k] = st; T[tail + k] = np.nan
        n_assoc[tail + k] = (1, 0, 0, 2)[k]
    status[tail + 4] = _abi.ROMAN_ST_MAXITER; status[tail + 5] = _abi.ROMAN_ST_TIE_FALLBACK | _abi.ROMAN_ST_ASSOC_TRUNCATED   # not failures
    cls = sa.Submap if in_place else FrameSubmap
    submaps = [[], []]
    sid = 0
    for r, n in ((0, S0), (1, S1)):
        for k in range(n):
            pose = np.eye(4)
            pose[:3, :3] = sa_rot(rng.uniform(-np.pi, np.pi), rng.normal(0, 0.05), rng.normal(0, 0.05))
            pose[:3, 3] = rng.uniform(-3, 3, 3)
            segs = [_Seg(100 * sid + q) for q in range(3)]
            submaps[r].append(cls(id=k, time=1000.0 * r + 10.0 * k, segments=segs, pose_flu=pose))
            sid += 1
    submaps[1][S1 - 1].time = submaps[0][S0 - 1].time + 1.0    # the last pair of the grid: inside the single-robot time gate
    n_assoc[B - 1] = THRESH + 5
    return dict(thresh_idx=tail + 6, dim=dim, B=B, S0=S0, S1=S1, T=T, n_assoc=n_assoc, status=status, submaps=submaps, tilt=tilt,
                upside_down=upside_down, rm_roll_pitch=rm_roll_pitch)


def case_params(case):
    from roman_amd.align import SubmapAlignParams
    p = SubmapAlignParams(dim=case["dim"], submap_radius=1e3, single_robot_lc=True, single_robot_lc_time_thresh=5.0,
                          force_rm_upside_down=case["upside_down"], force_rm_lc_roll_pitch=case["rm_roll_pitch"])
    io = sa.SubmapAlignIO(lc_association_thresh=THRESH)
    return p, io, StubRegistration(case["dim"], case["tilt"])


def planted_compute(case):
    """compute double for submap_align(): hands back the planted batch."""
    def compute(registration, batch):
        B = case["B"]
        assert len(batch) == B
        assoc = [np.zeros((int(case["n_assoc"][b]), 2), np.int32) for b in range(B)]
        return BatchResult(assoc, case["T"].copy(), case["status"].copy(), np.zeros(B, stats_dtype()))
    return compute


def per_pair_reference(case):
    """The existing per-pair code on the case: submap_align() pass 2 with the planted batch, loop_closure_edges(),
    transform_to_xyz_quat() -> (records, accepted) in the tail's terms, plus the result object."""
    import copy
    p, io, reg = case_params(case)
    submaps = copy.deepcopy(case["submaps"])
    res = sa.submap_align(p, submaps, io, registration=reg, compute=planted_compute(case))
    B, S1 = case["B"], case["S1"]
    rec = np.zeros(B, dtype=lc_record_dtype())
    rec["problem"] = np.arange(B)
    rec["n_assoc"] = res.clipper_num_associations.reshape(B).astype(np.int32)
    rec["T_hat"] = res.T_ij_hat_mat.reshape(B, 4, 4)
    rec["theta"] = np.deg2rad(res.clipper_angle_mat.reshape(B))      # submap_align stores |rad2deg(theta)|
    rec["dist"] = res.clipper_dist_mat.reshape(B)
    rec["edge_t"] = np.nan; rec["edge_q"] = np.nan
    acc = []
    for (i, j, T_edge) in sa.loop_closure_edges(res, submaps):
        b = i * S1 + j
        t, q = sa.transform_to_xyz_quat(T_edge)
        rec["edge_t"][b] = t; rec["edge_q"][b] = q; acc.append(b)
    return rec, np.array(acc, dtype=np.int32), res


def lc_inputs(case):
    """The tail's inputs for the case, built the way submap_align_grid builds them."""
    import copy
    p, io, reg = case_params(case)
    submaps = copy.deepcopy(case["submaps"])
    S0, S1, B = case["S0"], case["S1"], case["B"]
    Tw = [np.stack([np.array(sm.pose_gravity_aligned) for sm in submaps[r]]) for r in range(2)]     # pass 1 (in place or not)
    T_ref = np.matmul(np.linalg.inv(Tw[0])[:, None], Tw[1][None]).reshape(B, 4, 4)
    fr = [[sa._edge_frames(sm) for sm in submaps[r]] for r in range(2)]
    iL, iR = np.divmod(np.arange(B), S1)
    t0 = np.array([sm.time for sm in submaps[0]]); t1 = np.array([sm.time for sm in submaps[1]])
    enable = (~(np.abs(t0[iL] - t1[iR]) < p.single_robot_lc_time_thresh)).astype(np.int32)
    return LcInputs(dim=case["dim"], force_rm_upside_down=p.force_rm_upside_down, force_rm_lc_roll_pitch=p.force_rm_lc_roll_pitch,
                    tilt_thresh=TILT if case["tilt"] else None, lc_association_thresh=THRESH, T_ref=T_ref, enable=enable,
                    FL=np.stack([f[0] for f in fr[0]]), iL=iL, FR=np.stack([f[1] for f in fr[1]]), iR=iR)


ALL_CASES = [dict(dim=3, seed=1), dict(dim=3, seed=2, tilt=True), dict(dim=3, seed=3, upside_down=False, rm_roll_pitch=False),
             dict(dim=3, seed=4, tilt=True, upside_down=False), dict(dim=3, seed=5, in_place=True), dict(dim=2, seed=6)]


def host_reference_in_tail_terms(case):
    """per_pair_reference with the flags the per-pair code implies: it has no flag word, so ACCEPTED comes from the edge
    list and the failure kind from replaying its three checks per pair with its own (scipy) functions."""
    from scipy.spatial.transform import Rotation as Rot
    rec, acc, res = per_pair_reference(case)
    B = case["B"]
    flags = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if case["status"][b] & (_abi.ROMAN_ST_INSUFFICIENT | _abi.ROMAN_ST_EMPTY_MAP):
            flags[b] = _abi.ROMAN_LC_FAILED_INSUFFICIENT; continue
        if case["dim"] != 3:
            continue
        if case["tilt"]:
            _, pitch, roll = sa._zyx_euler(case["T"][b][:3, :3])
            if not (np.abs(roll) < TILT and np.abs(pitch) < TILT):
                flags[b] = _abi.ROMAN_LC_FAILED_TILT; continue
        if case["upside_down"]:
            rpy = Rot.from_matrix(case["T"][b][:3, :3]).as_euler('xyz')
            if np.abs(rpy[0]) > np.deg2rad(90.) or np.abs(rpy[1]) > np.deg2rad(90.):
                flags[b] = _abi.ROMAN_LC_FAILED_UPSIDE_DOWN
    failed_by_result = np.isnan(res.T_ij_hat_mat.reshape(B, 16)).all(axis=1)
    assert np.array_equal(failed_by_result, flags != 0)  # the replay names exactly the pairs submap_align() gave up on
    flags[acc] |= _abi.ROMAN_LC_ACCEPTED
    rec["flags"] = flags
    return rec, acc
