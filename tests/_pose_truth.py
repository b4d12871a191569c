"""tests/golden/pose_truth.npz (made by tests/golden/make_pose_truth.py): the rigid fit of point pairs at the edges of the pose code,
evaluated with mpmath on the exact float64 inputs — and the error measures that tests/test_gpu_pose_truth.py (the device) and
tests/test_pose_truth_cpu.py (the float64 reference restatement, oracle.t_align) share.

Units.  A fit (R, t) of a DETERMINED case is measured against the truth (R*, t*) in
    eR = |R - R*|_F / (2^-52 kappa (1 + c / r))        et = |t - t*| / (2^-52 kappa (1 + c / r) c)
kappa = s1 / (s2 + sgn(det H) s3) is the conditioning of the rotation against a perturbation of H (2-D: s1 / (s1 + sgn s2), at least
1), c the largest absolute coordinate, r the RMS radius of the centred cloud: a float64 coordinate carries an error of 2^-53 c, which is
a RELATIVE error of (c / r) 2^-53 of the centred cloud that H is made of.

K.  The bound on eR and et is not taken from the device.  REF_MAX is the largest of eR, et that oracle.t_align (numpy: pairwise sums,
LAPACK's SVD) reaches over the determined cases — 14.35, at scale_1e+06 (next: 10.6 at window_k193) — and
    K = 4 x REF_MAX rounded up to a power of two = 64;
the factor 4 is for another summation order (64 lane-strided partial sums against pairwise ones) and for Jacobi against LAPACK.
tests/test_pose_truth_cpu.py holds the reference to K / 4 = 16 on every run.
14.35 against 16 is a margin of a tenth, on a figure that belongs to the numpy / LAPACK build that measured it: another build may
round differently and miss K / 4 with nothing changed in this project.  K is not to be moved for that; measure again and look at
the family that moved (the normalisation, not the bound, is what a family may change).
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
REF_MAX = 14.35            # measured: max(eR, et) of oracle.t_align over the determined cases of the fixture (scale_1e+06: eR = 14.34)
K = 64                     # 4 x 14.35 = 57.4, rounded up to a power of two
assert K == 2 ** math.ceil(math.log2(4 * REF_MAX))
DETERMINED, UNDETERMINED, INSUFFICIENT = 0, 1, 2
FIELDS = ("m1", "m2", "H", "sv", "R", "t", "res", "kappa", "c", "r", "sgn")


def load():
    """The cases in batch order: dicts with tag, family, dim, k, kind, p1, p2 (k x dim) and the truth trimmed to dim."""
    z = np.load(os.path.join(GOLDEN, "pose_truth.npz"), allow_pickle=False)
    out = []
    for i in range(len(z["tag"])):
        d, k = int(z["dim"][i]), int(z["k"][i])
        lo, hi = int(z["off"][i]), int(z["off"][i + 1])
        c = dict(tag=str(z["tag"][i]), family=str(z["family"][i]), dim=d, k=k, kind=int(z["kind"][i]),
                 p1=z["p1"][lo:hi].reshape(k, d).copy(), p2=z["p2"][lo:hi].reshape(k, d).copy(), sgn=int(z["sgn"][i]))
        for name in ("m1", "m2", "sv", "t"):
            c[name] = z[name][i][:d].copy()
        for name in ("H", "R"):
            c[name] = z[name][i][:d, :d].copy()
        for name in ("res", "kappa", "c", "r"):
            c[name] = float(z[name][i])
        out.append(c)
    return out


def batch(cases, dim):
    """(indices into cases, p1, p2, offsets) of the ragged batch of one dimension, in fixture order."""
    idx = [i for i, c in enumerate(cases) if c["dim"] == dim]
    off = np.cumsum([0] + [cases[i]["k"] for i in idx]).astype(np.int64)
    return idx, np.concatenate([cases[i]["p1"] for i in idx]), np.concatenate([cases[i]["p2"] for i in idx]), off


def properness(R):
    """(|R'R - I|_F, |det R - 1|) in units of 2^-52."""
    return np.linalg.norm(R.T @ R - np.eye(len(R))) / EPS, abs(np.linalg.det(R) - 1.0) / EPS


def determined_errors(c, R, t):
    """(eR, et) of a fit of a DETERMINED case, in the units above."""
    unit = EPS * c["kappa"] * (1.0 + c["c"] / c["r"])
    return np.linalg.norm(R - c["R"]) / unit, np.linalg.norm(t - c["t"]) / (unit * c["c"])


def undetermined_errors(c, R, t):
    """(residual excess over the optimum in units of 2^-52 c sqrt(k), distance of the mapped centroid of p2 from the centroid of p1 in
    units of the translation bound with kappa = 1) of a fit of an UNDETERMINED case.  Where every p2 is the same point (r = 0) the
    (1 + c / r) factor, which stands for the error of R acting on the centroid, is left out: the stricter reading."""
    res = np.linalg.norm(c["p2"] @ R.T + t - c["p1"])
    f = 1.0 + c["c"] / c["r"] if c["r"] > 0 else 1.0
    return abs(res - c["res"]) / (EPS * c["c"] * math.sqrt(c["k"])), np.linalg.norm(R @ c["m2"] + t - c["m1"]) / (EPS * f * c["c"])
