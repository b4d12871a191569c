"""NumPy oracle of the frame data association scores: voxel IoU / IoM of point clouds, the cosine of their
descriptors, and the score and pair extraction of global_nearest_neighbor.  No device code.

Two forms of the geometric part:

LITERAL  the reference's VoxelGrid.from_points / .intersection / .iou [REF roman/map/voxel_grid.py:32-103] restated step by step:
         the float corners, a dense uint8 array of shape ((max_corner - min_corner) / vs + 2).astype(uint32), six slices and a
         product.  The one open3d call (VoxelGrid.create_from_point_cloud) is restated by open3d's documented rule
         (`o3d_grid_indices`); that line is UNPINNED against a real open3d.
SET      what the device computes: per cloud the sorted distinct GLOBAL keys min_corner_int + grid_index, per pair the number of
         keys both clouds hold inside [lo, hi) on every axis.

tests/test_voxel_oracle_cpu.py holds the two forms to each other; tests/test_assoc_golden_cpu.py holds the literal arithmetic to
values recorded from the reference's own VoxelGrid and global_nearest_neighbor."""
from types import SimpleNamespace

import numpy as np

M = 1e9                                   # [REF roman/map/global_nearest_neighbor.py:21]
OK, EMPTY, RANGE = 0, 1, 2                # ROMAN_ASSOC_OK / _EMPTY / _RANGE
IOU, IOM = 0, 1                           # ROMAN_ASSOC_IOU / _IOM
KEY_BIAS = 1 << 20                        # a key axis + KEY_BIAS must fit 21 bits


def params(voxel_size=0.2, geometric="iou", semantic=False, geo_range=(0.25, 1.0), sem_range=(0.8, 1.0)):
    return SimpleNamespace(voxel_size=float(voxel_size), geometric=geometric, semantic=bool(semantic),
                           geo_range=tuple(map(float, geo_range)), sem_range=tuple(map(float, sem_range)))


# ----------------------------------------------------------------------------------------------------------------- the shared lines
def corners(points, vs):
    """min_corner, max_corner as from_points forms them [REF voxel_grid.py:90-91] -> two (3,) float64."""
    return np.floor(np.min(points, axis=0) / vs) * vs, np.ceil(np.max(points, axis=0) / vs) * vs


def corner_int(corner, vs):
    """[REF voxel_grid.py:25-30]: astype(int64) TRUNCATES toward zero."""
    return (corner / vs).astype(np.int64)


def o3d_grid_indices(points, vs):
    """UNPINNED: open3d's documented rule for VoxelGrid.create_from_point_cloud — origin = min_bound - voxel_size * 0.5,
    grid_index = floor((p - origin) / voxel_size) per axis, one voxel per distinct index -> (k, 3) int64, lexicographic."""
    origin = np.min(points, axis=0) - vs * 0.5
    return np.unique(np.floor((points - origin) / vs).astype(np.int64), axis=0)


# ----------------------------------------------------------------------------------------------------------------- literal form
def literal_grid(points, vs):
    """VoxelGrid.from_points [REF voxel_grid.py:86-103] -> min_corner (1, 3), max_corner (1, 3), voxel_size, voxels (dense uint8)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    mn, mx = corners(points, vs)
    min_corner, max_corner = np.array([mn]), np.array([mx])
    idx = o3d_grid_indices(points, vs)
    voxels = np.zeros(((max_corner - min_corner) / vs + 2).astype(np.uint32).reshape(-1), dtype=np.uint8)
    voxels[idx[:, 0], idx[:, 1], idx[:, 2]] = 1          # an index outside the shape raises, as it would there
    return SimpleNamespace(min_corner=min_corner, max_corner=max_corner, voxel_size=vs, voxels=voxels)


def literal_volume(g):
    return np.sum(g.voxels) * g.voxel_size**3


def literal_intersection(a, b):
    """[REF voxel_grid.py:32-69]"""
    vs = a.voxel_size
    lo_f, hi_f = np.maximum(a.min_corner, b.min_corner), np.minimum(a.max_corner, b.max_corner)
    if np.any(lo_f >= hi_f):
        return 0.0
    a0, b0 = corner_int(a.min_corner, vs), corner_int(b.min_corner, vs)
    lo = np.maximum(a0, b0)
    hi = np.minimum(corner_int(a.max_corner, vs), corner_int(b.max_corner, vs))
    sub = []
    for g, g0 in ((a, a0), (b, b0)):
        sub.append(g.voxels[lo.item(0) - g0.item(0):hi.item(0) - g0.item(0),
                            lo.item(1) - g0.item(1):hi.item(1) - g0.item(1),
                            lo.item(2) - g0.item(2):hi.item(2) - g0.item(2)])
    assert sub[0].shape == sub[1].shape, "Subgrids do not have the same shape"
    return np.sum(sub[0] * sub[1]) * vs**3


def literal_iou(a, b, iom_as_iou=False):
    """[REF voxel_grid.py:75-83]"""
    inter = literal_intersection(a, b)
    va, vb = literal_volume(a), literal_volume(b)
    if iom_as_iou:
        if np.minimum(va, vb) == 0:
            return 0.0
        return inter / np.minimum(va, vb)
    if (va + vb - inter) == 0:
        return 0.0
    return inter / (va + vb - inter)


# ----------------------------------------------------------------------------------------------------------------- set form
def cloud_record(points, vs):
    """What the device keeps per cloud: status, the float corners, the truncated integer corners, and the sorted distinct global
    keys (k, 3).  EMPTY: no point.  RANGE: a coordinate is not finite, or a key axis + 2^20 does not fit 21 bits; such a cloud has
    no voxel.  (Both are this project's rules: the reference's from_points raises on an empty cloud.)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    none = np.zeros((0, 3), dtype=np.int64)
    if len(points) == 0:
        return SimpleNamespace(status=EMPTY, keys=none, n_vox=0, minc=np.zeros(3), maxc=np.zeros(3), mci=np.zeros(3, np.int64), maxci=np.zeros(3, np.int64))
    with np.errstate(all="ignore"):
        minc, maxc = corners(points, vs)
        origin = np.min(points, axis=0) - vs * 0.5
        t = np.trunc(minc / vs)
        top = t + np.floor((np.max(points, axis=0) - origin) / vs)          # the largest key of each axis
        fits = np.all(np.isfinite(points)) and np.all(t >= -KEY_BIAS) and np.all(top <= KEY_BIAS - 1)
    if not fits:
        return SimpleNamespace(status=RANGE, keys=none, n_vox=0, minc=minc, maxc=maxc, mci=np.zeros(3, np.int64), maxci=np.zeros(3, np.int64))
    mci, maxci = corner_int(minc, vs), corner_int(maxc, vs)
    keys = mci + o3d_grid_indices(points, vs)
    return SimpleNamespace(status=OK, keys=keys, n_vox=len(keys), minc=minc, maxc=maxc, mci=mci, maxci=maxci)


def set_intersection(a, b):
    """The number of keys both clouds hold with lo <= key < hi on every axis; 0 where the float boxes fail the reference's test."""
    if a.n_vox == 0 or b.n_vox == 0:
        return 0
    if np.any(np.maximum(a.minc, b.minc) >= np.minimum(a.maxc, b.maxc)):
        return 0
    lo, hi = np.maximum(a.mci, b.mci), np.minimum(a.maxci, b.maxci)
    ka = {tuple(k) for k in a.keys.tolist() if all(lo[x] <= k[x] < hi[x] for x in range(3))}
    return sum(1 for k in b.keys.tolist() if tuple(k) in ka)


def padding_keys(rec):
    """The keys of a cloud outside its own [min_corner_int, max_corner_int): they count in the volume, never in an intersection."""
    k = rec.keys
    return k[np.any((k < rec.mci) | (k >= rec.maxci), axis=1)]


def geo_from_counts(na, nb, inter, vs, method):
    """IoU / IoM from integer counts in the reference's operation order [REF voxel_grid.py:22, :69, :75-83]."""
    va, vb, iv = np.float64(na) * vs**3, np.float64(nb) * vs**3, np.float64(inter) * vs**3
    if method in (IOM, "iom"):
        m = np.minimum(va, vb)
        return 0.0 if m == 0 else float(iv / m)
    den = va + vb - iv
    return 0.0 if den == 0 else float(iv / den)


# ----------------------------------------------------------------------------------------------------------------- score
def cosine(da, db):
    """[REF roman/map/mapper.py:204-212]: a None descriptor on either side gives 1.0."""
    if da is None or db is None:
        return 1.0
    with np.errstate(all="ignore"):
        return float(np.dot(da, db) / (np.linalg.norm(da) * np.linalg.norm(db)))


def score_of(geo, sem, p, sqrt=False):
    """[REF roman/map/global_nearest_neighbor.py:25-36]; sem None: one criterion.  sqrt=True: the device's correctly rounded
    square root in place of np.power(x, 1 / 2)."""
    if sem is None:
        similarity, rng = np.float64(geo), np.array(p.geo_range).reshape(2, 1)
    else:
        similarity, rng = np.array([geo, sem]), np.array([p.geo_range, p.sem_range]).T
    with np.errstate(all="ignore"):
        if np.any(similarity < rng[0, :]):
            return M
        if isinstance(similarity, np.ndarray):
            sim_norm = (similarity - rng[0, :]) / (rng[1, :] - rng[0, :])
            prod = np.prod(sim_norm)
            return float(-np.sqrt(prod)) if sqrt else float(-np.power(prod, 1.0 / len(similarity)))
        return float(-similarity)


def scores(clouds_a, clouds_b, p, desc_a=None, desc_b=None):
    """The set form over lists of (n, 3) clouds; clouds_b None: self mode.  desc_*: (N, d) arrays or None (no descriptors: sem is
    1.0 when p.semantic).  -> n_vox, status (per cloud, rows then columns), inter, geo, sem, score (N1 x N2)."""
    vs = p.voxel_size
    ra = [cloud_record(c, vs) for c in clouds_a]
    self_mode = clouds_b is None
    rb = ra if self_mode else [cloud_record(c, vs) for c in clouds_b]
    if self_mode:
        desc_b = desc_a
    n1, n2 = len(ra), len(rb)
    inter = np.zeros((n1, n2), dtype=np.int32); geo = np.zeros((n1, n2)); sem = np.ones((n1, n2)); score = np.zeros((n1, n2))
    for i in range(n1):
        for j in range(n2):
            inter[i, j] = set_intersection(ra[i], rb[j])
            geo[i, j] = geo_from_counts(ra[i].n_vox, rb[j].n_vox, inter[i, j], vs, p.geometric)
            if p.semantic:
                sem[i, j] = cosine(None if desc_a is None else desc_a[i], None if desc_b is None else desc_b[j])
            score[i, j] = score_of(geo[i, j], sem[i, j] if p.semantic else None, p)
    recs = ra if self_mode else ra + rb
    return SimpleNamespace(n_vox=np.array([r.n_vox for r in recs], dtype=np.int32), status=np.array([r.status for r in recs], dtype=np.int32),
                           inter=inter, geo=geo, sem=sem if p.semantic else None, score=score)


def literal_scores(clouds_a, clouds_b, p, desc_a=None, desc_b=None):
    """The reference's loop with the literal grids: similarity_fun per pair, then the score rule -> geo, score (N1 x N2).
    Every cloud must hold a point."""
    vs = p.voxel_size
    ga = [literal_grid(c, vs) for c in clouds_a]
    gb = ga if clouds_b is None else [literal_grid(c, vs) for c in clouds_b]
    if clouds_b is None:
        desc_b = desc_a
    geo = np.zeros((len(ga), len(gb))); score = np.zeros((len(ga), len(gb)))
    for i, a in enumerate(ga):
        for j, b in enumerate(gb):
            geo[i, j] = literal_iou(a, b, iom_as_iou=p.geometric in (IOM, "iom"))
            sem = cosine(None if desc_a is None else desc_a[i], None if desc_b is None else desc_b[j]) if p.semantic else None
            score[i, j] = score_of(geo[i, j], sem, p)
    return geo, score


def gnn_pairs(score):
    """The augmented cost matrix and the pair extraction [REF roman/map/global_nearest_neighbor.py:38-50] -> [(i, j), ...]."""
    from scipy.optimize import linear_sum_assignment
    score = np.asarray(score, dtype=np.float64)
    n1, n2 = score.shape
    cost = np.concatenate([np.concatenate([score, np.ones(score.shape)], axis=1), np.ones((n1, 2 * n2))], axis=0)
    rows, cols = linear_sum_assignment(cost)
    return [(int(i), int(j)) for i, j in zip(rows, cols) if i < n1 and j < n2]
