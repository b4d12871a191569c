"""CPU oracle of roman_segment_cluster — TEST INFRASTRUCTURE.

What Segment.final_cleanup does to a cloud [REF roman/object/segment.py:195-220]: open3d's cluster_dbscan(eps, min_points), then
"keep the largest cluster".  open3d is not installed: its call is restated from its published source, in TWO forms that
tests/test_dbscan_oracle_cpu.py holds to each other.  UNPINNED against a real open3d: the rounding of d2, the strict radius
comparison, and the closed form of the label order.

  neighbours         d2(i, j) = (dx dx + dy dy) + dz dz in double, no contraction; j is a neighbour of i iff d2 < eps * eps
                     (strict: nanoflann's radius result set), eps * eps formed once; every point is its own neighbour
  labels_sequential  open3d's loop, literally: neighbour lists first; labels start at -2 (undefined); the outer index ascends; a
                     point with fewer than min_points neighbours becomes -1 (noise); otherwise it opens a cluster, and a
                     frontier SET of its neighbours is expanded until empty — a noise point the cluster reaches is relabelled
                     (and not expanded), an undefined one is labelled and, if it is a core point, its neighbours join the frontier
  labels_closed      rules 1-4 of the C header: core flags; clusters = connected components of the core points, labelled in
                     ascending order of their smallest core index; a border point takes the smallest label among its core
                     neighbours; the rest is noise
  final_cleanup      n_clusters = max(label) + 1, sizes over core and border members, np.argmax (the lowest label among equals),
                     the kept points in input order; no cluster -> no point (the reference raises, the mapper drops the segment)
"""
from types import SimpleNamespace

import numpy as np

OK, EMPTY, RANGE = 0, 1, 2                # ROMAN_ASSOC_OK / _EMPTY / _RANGE


def d2_matrix(points):
    """(n, n) squared distances in the pinned expression: (dx dx + dy dy) + dz dz, every operation rounded once."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    dx = p[:, None, 0] - p[None, :, 0]
    dy = p[:, None, 1] - p[None, :, 1]
    dz = p[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbours(points, eps):
    """(n, n) bool: d2 < eps * eps"""
    return d2_matrix(points) < np.float64(eps) * np.float64(eps)


def neighbour_lists(points, eps, block=1024):
    """every point's neighbours, ascending; the same arithmetic as d2_matrix, `block` rows at a time (a large cloud's matrix is never whole)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    e2 = np.float64(eps) * np.float64(eps)
    out = []
    for r0 in range(0, len(p), block):
        q = p[r0:r0 + block]
        dx, dy, dz = (q[:, None, k] - p[None, :, k] for k in range(3))
        out += [np.flatnonzero(r) for r in ((dx * dx + dy * dy) + dz * dz < e2)]
    return out


def labels_sequential(points, eps, min_points):
    """open3d's ClusterDBSCAN loop as published, over precomputed neighbour lists."""
    nbs = neighbour_lists(points, eps)
    n = len(nbs)
    labels = np.full(n, -2, dtype=np.int32)
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            labels[idx] = -1
            continue
        frontier = set(int(v) for v in nbs[idx])       # nbs_next
        visited = {idx}                                # nbs_visited
        labels[idx] = cluster
        while frontier:
            nb = frontier.pop()
            visited.add(nb)
            if labels[nb] == -1:                       # noise that a later cluster reaches: a border point of that cluster
                labels[nb] = cluster
            if labels[nb] != -2:
                continue
            labels[nb] = cluster
            if len(nbs[nb]) >= min_points:
                for qnb in nbs[nb]:
                    if int(qnb) not in visited:
                        frontier.add(int(qnb))
        cluster += 1
    return labels


def core_flags(points, eps, min_points):
    return neighbours(points, eps).sum(axis=1) >= min_points


def labels_closed(points, eps, min_points):
    """Rules 1-4: components of the core points by a plain union-find, labelled by smallest core index; borders by minimum."""
    nb = neighbours(points, eps)
    n = len(nb)
    core = nb.sum(axis=1) >= min_points
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i in np.flatnonzero(core):
        for j in np.flatnonzero(nb[i] & core):
            if j < i:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.array([find(i) if core[i] else -1 for i in range(n)], dtype=np.int64)
    roots = sorted(set(int(r) for r in root[core]))
    rank = {r: k for k, r in enumerate(roots)}
    labels = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = rank[int(root[i])]
        else:
            near = np.flatnonzero(nb[i] & core)
            if len(near):
                labels[i] = min(rank[int(root[j])] for j in near)
    return labels


def final_cleanup(points, eps, min_points=10, labels=None):
    """-> status, labels (None unless OK), n_clusters, kept, points (count, 3) — what roman_segment_cluster writes for one job."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0:
        return SimpleNamespace(status=EMPTY, labels=None, n_clusters=0, kept=-1, points=np.zeros((0, 3)))
    if not np.all(np.isfinite(p)):
        return SimpleNamespace(status=RANGE, labels=None, n_clusters=0, kept=-1, points=np.zeros((0, 3)))
    lab = labels_closed(p, eps, min_points) if labels is None else labels
    n_clusters = int(lab.max()) + 1
    if n_clusters == 0:                        # np.argmax of an empty array raises in the reference; the mapper drops the segment
        return SimpleNamespace(status=OK, labels=lab, n_clusters=0, kept=-1, points=np.zeros((0, 3)))
    sizes = np.array([np.sum(lab == k) for k in range(n_clusters)])
    kept = int(np.argmax(sizes))
    return SimpleNamespace(status=OK, labels=lab, n_clusters=n_clusters, kept=kept, points=np.ascontiguousarray(p[lab == kept]))


def edge_gap_ulps(points, eps):
    """The smallest distance, in ulps of eps * eps, between a d2 of the cloud and eps * eps."""
    e2 = np.float64(eps) * np.float64(eps)
    return float(np.min(np.abs(d2_matrix(points) - e2)) / np.spacing(e2))
