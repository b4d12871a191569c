"""NumPy oracle of the segment update: what Segment._add_points and _cleanup_points do to a segment's cloud
[REF roman/object/segment.py:133-193], restated line by line.  No device code — TEST INFRASTRUCTURE.

open3d is not installed, so its two calls are restated from its documented and published behaviour; both are UNPINNED against a
real open3d.  What the restatement ASSUMES:

  voxel_down_sample(vs)               voxel_min_bound = min_bound - 0.5 vs; index = int(floor((p - voxel_min_bound) / vs)) per axis;
                                      one output point per distinct index: the sum of the index's points, added one after another
                                      in input order from 0.0 (open3d's AccumulatedPoint), divided by double(count).  open3d emits
                                      the voxels in the order of its hash map; here the order is ASCENDING VOXEL KEY (x most
                                      significant) — our own rule, which affects only the summation order of the threshold.
  remove_statistical_outlier(10, r)   per point the min(10, m) nearest of all m points, ITSELF INCLUDED (distance 0), by squared
                                      distance (dx dx + dy dy) + dz dz; the square roots are added ascending from 0.0 and divided
                                      by their number: avg_i.  mean = sum(avg_i, avg_i > 0) / m; std = sqrt(sum((avg_i - mean)^2,
                                      avg_i > 0) / (m - 1)); thr = mean + r std; point i is kept iff avg_i > 0 and avg_i < thr.
                                      (open3d divides by the number of points that found a neighbour; every point finds itself,
                                      so that number is m.)  The two sums over m are taken in the device's fixed order (`fixed_sum`).

Two forms of the down-sample are held to each other by tests/test_integrate_oracle_cpu.py: `down_sample` (sort by (key, input
index), then the runs) and `down_sample_literal` (a dict of accumulators filled in input order)."""
from types import SimpleNamespace

import numpy as np

OK, EMPTY, RANGE = 0, 1, 2                # ROMAN_ASSOC_OK / _EMPTY / _RANGE (§4.25's vocabulary)
NEIGHBORS = 10                            # [REF roman/object/segment.py:183-184]
KEY_TOP = (1 << 21) - 1                   # the largest voxel index an axis of the key holds
EPS = 2.0 ** -53


def params(voxel_size=0.05, outlier_std=1.0):
    """SegmentParams [REF roman/params/mapper_params.py:96-103]: a deviation that is <= 0 or infinite is None."""
    std = None if (outlier_std is None or not np.isfinite(outlier_std) or outlier_std <= 0) else float(outlier_std)
    return SimpleNamespace(voxel_size=float(voxel_size), outlier_std=std)


# ----------------------------------------------------------------------------------------------------------------- 1. assemble
def world_points(points, pose):
    """R p + t, each row ((r0 x + r1 y) + r2 z) + t [REF roman/object/segment.py:142-147].  The reference's `Rwb @ points` goes
    through BLAS; its rounding is UNPINNED."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if pose is None:
        return p.copy()
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


# ----------------------------------------------------------------------------------------------------------------- 2. down-sample
def voxel_indices(points, vs):
    """-> (n, 3) int64 voxel indices, or None: a coordinate is not finite or an index needs more than 21 bits (status RANGE)."""
    with np.errstate(all="ignore"):
        if not np.all(np.isfinite(points)):
            return None
        origin = np.min(points, axis=0) - 0.5 * vs
        if np.any(np.floor((np.max(points, axis=0) - origin) / vs) > KEY_TOP):
            return None
        return np.floor((points - origin) / vs).astype(np.int64)


def pack(idx):
    return (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]


def down_sample(points, vs):
    """-> (m, 3) in ascending voxel key, or None (RANGE).  Sort by (key, input index); add every run in index order from 0.0."""
    idx = voxel_indices(points, vs)
    if idx is None:
        return None
    key = pack(idx)
    order = np.lexsort((np.arange(len(key)), key))
    key, pts = key[order], points[order]
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    count = np.diff(np.concatenate([head, [len(key)]]))
    acc = np.zeros((len(head), 3))
    for r in range(int(count.max())):                     # the r-th point of every run that has one: the order inside a run is kept
        has = count > r
        acc[has] = acc[has] + pts[head[has] + r]
    return acc / count.astype(np.float64)[:, None]


def down_sample_literal(points, vs):
    """open3d's loop: a map from voxel index to AccumulatedPoint, filled point by point; emitted in ascending key."""
    origin = np.min(points, axis=0) - 0.5 * vs
    cells = {}
    for p in points:
        ref = (p - origin) / vs
        ix = (int(np.floor(ref[0])), int(np.floor(ref[1])), int(np.floor(ref[2])))
        a = cells.setdefault(ix, [0.0, 0.0, 0.0, 0])
        a[0] += p[0]; a[1] += p[1]; a[2] += p[2]; a[3] += 1
    return np.array([[a[0] / float(a[3]), a[1] / float(a[3]), a[2] / float(a[3])] for _, a in sorted(cells.items())]).reshape(-1, 3)


# ----------------------------------------------------------------------------------------------------------------- 3. neighbour distances
def mean_neighbor_distances(pts):
    """avg (m,): the mean distance of every point to its min(10, m) nearest of all m, itself included."""
    m = len(pts)
    k = min(NEIGHBORS, m)
    avg = np.zeros(m)
    for a in range(0, m, 512):
        q = pts[a:a + 512]
        dx, dy, dz = (q[:, None, c] - pts[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        near = np.sqrt(np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1))
        s = np.zeros(len(q))
        for r in range(k):                                # ascending, from 0.0
            s = s + near[:, r]
        avg[a:a + 512] = s / float(k)
    return avg


# ----------------------------------------------------------------------------------------------------------------- 4. threshold
def fixed_sum(v):
    """The fixed order of the two sums over m: lane l of 64 adds the elements l, l + 64, ... one after another
    from 0.0; then the xor butterfly 32, 16, 8, 4, 2, 1 (lane l adds lane l ^ off).  Every lane ends with the same bits."""
    v = np.asarray(v, dtype=np.float64)
    rows = np.concatenate([v, np.zeros(-len(v) % 64)]).reshape(-1, 64)
    s = np.zeros(64)
    for row in rows:
        s = s + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ off]
    return float(s[0])


def sum_depth(m):
    """Additions on the longest path of fixed_sum over m terms."""
    return max(-(-m // 64) - 1, 0) + 6


def threshold(avg, std_ratio):
    m = len(avg)
    pos = avg > 0
    with np.errstate(all="ignore"):
        mean = np.float64(fixed_sum(np.where(pos, avg, 0.0))) / np.float64(m)
        sq = np.float64(fixed_sum(np.where(pos, (avg - mean) * (avg - mean), 0.0)))
        return float(mean + np.float64(std_ratio) * np.sqrt(sq / np.float64(m - 1)))          # m - 1 == 0: 0 / 0, a NaN threshold


def threshold_truth(avg, std_ratio):
    """The same formula in np.longdouble, any order -> (thr, bound): bound is what the float64 evaluation in fixed_sum's order may
    differ by.  With u = 2^-53, D = sum_depth(m), every avg_i > 0 (or 0):
      mean      D additions and a division: |d mean| <= (D + 1) u mean =: em
      sq        a term (a - mean^)^2 carries 3 roundings and moves by 2 |a - mean| em + em^2 with the mean; over the sum (Cauchy-
                Schwarz) |d sq| <= (D + 3) u sq + 2 em sqrt(m sq) + m em^2 =: eq
      std       a division and a square root: |d std| <= min(eq / (2 (m - 1) std), sqrt(eq / (m - 1))) + 2 u std =: es
      thr       a product and a sum: |d thr| <= em + r (es + u std) + u |thr|
    times 1 + 2^-4 for the terms of second order."""
    m = len(avg)
    if m < 2:
        return np.nan, np.nan
    a = avg.astype(np.longdouble)
    pos = a > 0
    mean = a[pos].sum() / m
    sq = ((a[pos] - mean) ** 2).sum()
    std = np.sqrt(sq / (m - 1))
    thr = mean + np.longdouble(std_ratio) * std
    D = sum_depth(m)
    mean, sq, std, thr = float(mean), float(sq), float(std), float(thr)
    em = (D + 1) * EPS * mean
    eq = (D + 3) * EPS * sq + 2.0 * em * np.sqrt(m * sq) + m * em * em
    es = min(eq / (2.0 * (m - 1) * std) if std > 0 else np.inf, np.sqrt(eq / (m - 1))) + 2.0 * EPS * std
    return thr, (em + std_ratio * (es + EPS * std) + EPS * abs(thr)) * (1.0 + 2.0 ** -4)


# ----------------------------------------------------------------------------------------------------------------- the whole job
def cleanup(points, P):
    """_cleanup_points [REF roman/object/segment.py:177-193] on a non-empty cloud -> SimpleNamespace(points (count, 3), status,
    down (m, 3) the down-sampled cloud, avg (m,) and thr (None without the outlier step))."""
    down = down_sample(points, P.voxel_size)
    if down is None:
        return SimpleNamespace(points=np.zeros((0, 3)), status=RANGE, down=np.zeros((0, 3)), avg=None, thr=None)
    if P.outlier_std is None:
        return SimpleNamespace(points=down, status=OK, down=down, avg=None, thr=None)
    avg = mean_neighbor_distances(down)
    thr = threshold(avg, P.outlier_std)
    keep = (avg > 0) & (avg < thr)
    return SimpleNamespace(points=down[keep], status=OK, down=down, avg=avg, thr=thr)


def integrate(base, add, pose, P):
    """One job: `base` (nb, 3) or None (a new segment), `add` (na, 3) and its pose or None.  An empty added cloud returns the base
    unchanged, with no clean-up [REF roman/object/segment.py:165-166]."""
    base = np.zeros((0, 3)) if base is None else np.asarray(base, dtype=np.float64).reshape(-1, 3)
    add = np.asarray(add, dtype=np.float64).reshape(-1, 3)
    if len(add) == 0:
        return SimpleNamespace(points=base.copy(), status=OK if len(base) else EMPTY, down=base.copy(), avg=None, thr=None)
    return cleanup(np.concatenate([base, world_points(add, pose)], axis=0), P)


# ----------------------------------------------------------------------------------------------------------------- the descriptor
class Descriptor:
    """The semantic descriptor of a segment as _add_semantic_descriptor keeps it [REF roman/object/segment.py:474-489], line by
    line: the first descriptor over its norm with count 1; later the mean weighted by the counts, the added descriptor over its
    norm; and after EITHER, the stored descriptor over its own norm (:489)."""
    def __init__(self):
        self.value, self.cnt = None, 0

    def add(self, descriptor, cnt=1):
        if descriptor is None:
            return self
        if self.value is None:
            assert cnt == 1
            self.value = descriptor / np.linalg.norm(descriptor)
            self.cnt = cnt
        else:
            self.value = (self.value * self.cnt / (self.cnt + cnt) + descriptor * cnt / np.linalg.norm(descriptor) / (self.cnt + cnt))
            self.cnt += cnt
        self.value = self.value / np.linalg.norm(self.value)
        return self
