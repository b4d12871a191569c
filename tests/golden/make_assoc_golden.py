"""Writes tests/golden/assoc_golden.npz from the REFERENCE's own code: VoxelGrid.iou (both methods) and global_nearest_neighbor.

    python tests/golden/make_assoc_golden.py /path/to/the/reference/checkout

voxel_grid.py needs open3d only at import (its from_points is the one function that calls it), so an empty stand-in module named
`open3d` is registered first; global_nearest_neighbor.py needs numpy and scipy.  The VoxelGrid objects are built with the
reference's constructor from the arrays of tests/_voxel_oracle.literal_grid — the restatement of from_points whose open3d line is
UNPINNED — so the file pins intersection, IoU, IoM, the score rule and the pair extraction against the reference itself.  The
file holds data only: per scene the clouds, the voxel size, the ranges, and what the reference returned."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _voxel_oracle as vo  # noqa: E402


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenes():
    """(voxel size, row clouds, column clouds, geo range, sem range or None, descriptors or None)"""
    rng = np.random.default_rng(77)
    for vs, n1, n2, spread, sem in ((0.2, 4, 5, 0.3, False), (0.05, 3, 3, 0.07, True), (1.0, 5, 2, 1.5, False), (0.2, 3, 4, 0.25, True), (0.2, 2, 2, 30.0, False)):
        centres = rng.uniform(-2.0, 2.0, (n1, 3)) * spread * 0.5
        rows = [c + rng.normal(size=(int(rng.integers(4, 20)), 3)) * spread for c in centres]
        cols = [rows[k % n1][k // n1::2] + rng.normal(size=3) * (0.1 + 0.2 * (k // n1)) * spread for k in range(n2)]   # an observation: part of a row's cloud, displaced
        desc = rng.normal(size=(n1 + n2, 6)) if sem else None
        if sem:                                             # columns resemble their rows, so that some pairs pass the semantic threshold
            desc[n1:] = desc[np.arange(n2) % n1] + 0.2 * rng.normal(size=(n2, 6))
        yield vs, rows, cols, (0.25, 1.0) if vs != 1.0 else (0.1, 0.9), (0.8, 1.0) if sem else None, desc


def main(ref):
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    VoxelGrid = load(ref, "roman/map/voxel_grid.py", "ref_voxel_grid").VoxelGrid
    gnn = load(ref, "roman/map/global_nearest_neighbor.py", "ref_gnn").global_nearest_neighbor
    out = {}
    n = 0
    for vs, rows, cols, geo_range, sem_range, desc in scenes():
        grid = lambda p: (lambda g: VoxelGrid(g.min_corner, g.max_corner, g.voxel_size, g.voxels))(vo.literal_grid(p, vs))
        ga, gb = [grid(p) for p in rows], [grid(p) for p in cols]
        iou = np.array([[a.iou(b) for b in gb] for a in ga], dtype=np.float64)
        iom = np.array([[a.iou(b, iom_as_iou=True) for b in gb] for a in ga], dtype=np.float64)
        inter = np.array([[a.intersection(b) for b in gb] for a in ga], dtype=np.float64)
        n1 = len(rows)
        for method, geo in (("iou", iou), ("iom", iom)):
            if sem_range is None:
                fun = lambda i, j, geo=geo: geo[i, j]
                rng_ = np.array(geo_range).reshape(2, 1)
            else:
                fun = lambda i, j, geo=geo: np.array([geo[i, j], vo.cosine(desc[i], desc[n1 + j])])
                rng_ = np.array([geo_range, sem_range]).T
            pairs = gnn(list(range(n1)), list(range(len(cols))), fun, rng_)
            out[f"pairs_{method}_{n}"] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
        out[f"vs_{n}"] = np.float64(vs)
        out[f"points_{n}"] = np.vstack(rows + cols)
        out[f"off_{n}"] = np.concatenate([[0], np.cumsum([len(p) for p in rows + cols])]).astype(np.int64)
        out[f"n1_{n}"] = np.int64(n1)
        out[f"geo_range_{n}"] = np.array(geo_range)
        out[f"sem_range_{n}"] = np.array(sem_range if sem_range else [])
        out[f"desc_{n}"] = desc if desc is not None else np.zeros((0, 0))
        out[f"iou_{n}"], out[f"iom_{n}"], out[f"inter_{n}"] = iou, iom, inter
        n += 1
    out["n"] = np.int64(n)
    np.savez_compressed(os.path.join(HERE, "assoc_golden.npz"), **out)
    print(f"{n} scenes -> assoc_golden.npz")


if __name__ == "__main__":
    main(sys.argv[1])
