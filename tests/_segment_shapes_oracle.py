"""NumPy oracle of the segment-shape step — TEST INFRASTRUCTURE.

Per segment, what Segment.minimal_data() reads [REF roman/object/segment.py:496-508]:
  centre      'mean': the mean [REF :271-272]; 'bottom_middle': np.median of x and y, np.min of z [REF :267-270]
  ratios      (e0 - e1) / e0, (e1 - e2) / e0, e2 / e0 [REF :445-472] of the singular values of the covariance [REF :441]
  extent      of the box in the covariance's eigenframe, ascending; volume their product; n <= 4: zeros [REF :253, :260]
The mean and the CENTRED covariance sum (x - m)(x - m)' / n are computed in np.longdouble (the stated deviation from open3d's
one-pass form); the eigen-decomposition is np.linalg.eigh of the float64 rounding of that covariance; the box is
taken in that eigenframe.  `reference_formulas` is the reference's own arithmetic (float64 one-pass covariance, np.linalg.svd)."""
import numpy as np

EPS = 2.0 ** -53
JACOBI_C = 64          # roundings the device's cyclic Jacobi adds to an eigenvalue, in units of 2^-53 e0: at most 6 sweeps x 3 rotations,
                       # each a backward error of about 3 roundings of |C|, plus the oracle's own eigh


def sum_depth(n, block_min):
    """Depth of the device's fixed summation tree over n terms (kernels.hip.h): thread t of a team of NW waves adds its terms one
    after the other (ceil(n / (64 NW)) - 1 additions), wave_sum63 adds 6 levels, the NW waves' sums are added in wave order."""
    nw = 4 if n >= block_min else 1
    return max(-(-n // (64 * nw)) - 1, 0) + 6 + (nw - 1)


def segment(points, center_ref="mean"):
    """-> dict(center (3,), ratios (3,), extent (3,) ascending, volume, eig (3,) descending, cov (3, 3), mean (3,))"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if n == 0:
        z = np.zeros(3)
        return dict(center=z, ratios=z.copy(), extent=z.copy(), volume=0.0, eig=z.copy(), cov=np.zeros((3, 3)), mean=z.copy())
    pl = p.astype(np.longdouble)
    mean_l = pl.sum(axis=0) / np.longdouble(n)
    d = pl - mean_l
    cov = ((d.T @ d) / np.longdouble(n)).astype(np.float64)
    mean = mean_l.astype(np.float64)
    w, V = np.linalg.eigh(cov)
    order = np.argsort(-np.abs(w), kind="stable")
    e, V = np.abs(w)[order], V[:, order]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = np.array([(e[0] - e[1]) / e[0], (e[1] - e[2]) / e[0], e[2] / e[0]])
    if n > 4:
        proj = (d.astype(np.float64)) @ V
        extent = np.sort(proj.max(axis=0) - proj.min(axis=0))
    else:
        extent = np.zeros(3)
    if center_ref == "bottom_middle":
        center = np.median(p, axis=0)                            # [REF roman/object/segment.py:268]
        center[2] = np.min(p[:, 2])                              # [REF :269]
    else:
        center = mean
    return dict(center=center, ratios=ratios, extent=extent, volume=float(extent[0] * extent[1] * extent[2]), eig=e, cov=cov, mean=mean)


def reference_formulas(points):
    """The reference's arithmetic in float64: open3d's one-pass covariance E[xx'] - mm' [REF roman/object/segment.py:430], the singular
    values normalised to sum one [REF :441-442], the three ratios [REF :445-472] -> (mean, cov, ratios)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    mean = p.sum(axis=0) / n
    cov = (p.T @ p) / n - np.outer(mean, mean)
    _, s, _ = np.linalg.svd(cov)
    e = s / s.sum()
    return mean, cov, np.array([(e[0] - e[1]) / e[0], (e[1] - e[2]) / e[0], e[2] / e[0]])


def bounds(points, block_min):
    """The error bounds of the device's values against `segment(points)`, from the summation order (module docstring of
    tests/test_gpu_segment_shapes.py) -> dict(center (3,), ratio, extent, volume)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    o = segment(p)
    D = sum_depth(n, block_min)
    center = (D + 1) * EPS * np.abs(p).sum(axis=0) / n + 2.0 ** -1074
    d = p - o["mean"]
    tr = float((d * d).sum() / n)                                # sum |term| / n over the diagonal sums: the trace
    d_eig = ((D + 4) * tr + JACOBI_C * o["eig"][0]) * EPS        # |delta e_k| <= ||delta C||_F + the Jacobi sweeps
    ratio = 3.0 * d_eig / o["eig"][0] if o["eig"][0] > 0 else np.nan
    e = o["eig"]
    gap = min(e[0] - e[1], e[1] - e[2])
    size = float(np.linalg.norm(d, axis=1).max()) if n else 0.0
    # a box side: 8 roundings of the projections, plus the turn of the eigenframe (Davis-Kahan: sin <= ||delta C|| / gap) times the
    # cloud's radius, both ends of the side
    extent = (8 * EPS * size + 2.0 * size * (2.0 * d_eig / gap)) if gap > 0 else np.inf
    volume = np.inf if not np.isfinite(extent) else extent * (o["extent"][0] * o["extent"][1] + o["extent"][0] * o["extent"][2] + o["extent"][1] * o["extent"][2]) * 1.01
    return dict(center=center, ratio=ratio, extent=extent, volume=volume)
