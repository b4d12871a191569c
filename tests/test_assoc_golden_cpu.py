"""tests/_voxel_oracle.py against tests/golden/assoc_golden.npz — values the REFERENCE's own VoxelGrid.iou / .intersection and
global_nearest_neighbor returned (tests/golden/make_assoc_golden.py) — no GPU.  This pins the oracle's intersection, IoU, IoM,
score rule and pair extraction to the reference; only the open3d voxelisation line stays unpinned."""
import os

import numpy as np
import pytest

import _voxel_oracle as vo
from conftest import GOLDEN


def cases():
    z = np.load(os.path.join(GOLDEN, "assoc_golden.npz"), allow_pickle=False)
    out = []
    for i in range(int(z["n"])):
        off, pts, n1 = z[f"off_{i}"], z[f"points_{i}"], int(z[f"n1_{i}"])
        clouds = [pts[off[k]:off[k + 1]] for k in range(len(off) - 1)]
        sem_range = z[f"sem_range_{i}"]
        desc = z[f"desc_{i}"]
        out.append(dict(vs=float(z[f"vs_{i}"]), rows=clouds[:n1], cols=clouds[n1:], geo_range=tuple(z[f"geo_range_{i}"]),
                        sem_range=tuple(sem_range) if len(sem_range) else None, desc=desc if desc.size else None,
                        iou=z[f"iou_{i}"], iom=z[f"iom_{i}"], inter=z[f"inter_{i}"],
                        pairs={m: [tuple(p) for p in z[f"pairs_{m}_{i}"].tolist()] for m in ("iou", "iom")}))
    return out


CASES = cases()


def test_the_golden_file_is_worth_its_name():
    assert len(CASES) >= 5
    assert sum(int(np.count_nonzero(c["inter"])) for c in CASES) > 10
    assert any(c["sem_range"] is not None for c in CASES)
    assert any(len(c["pairs"]["iou"]) == 0 for c in CASES) and any(len(c["pairs"]["iom"]) >= 3 for c in CASES)
    assert any(c["pairs"]["iou"] != c["pairs"]["iom"] for c in CASES)


@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("method", ["iou", "iom"])
def test_oracle_matches_the_reference(k, method):
    c = CASES[k]
    n1 = len(c["rows"])
    p = vo.params(c["vs"], method, c["sem_range"] is not None, c["geo_range"], c["sem_range"] or (0.8, 1.0))
    da, db = (None, None) if c["desc"] is None else (c["desc"][:n1], c["desc"][n1:])
    r = vo.scores(c["rows"], c["cols"], p, da, db)
    assert np.array_equal(r.inter * c["vs"]**3, c["inter"])
    assert r.geo.tobytes() == c[method].tobytes()
    geo_l, score_l = vo.literal_scores(c["rows"], c["cols"], p, da, db)
    assert geo_l.tobytes() == c[method].tobytes()
    assert np.array_equal(score_l, r.score, equal_nan=True)
    assert vo.gnn_pairs(r.score) == c["pairs"][method]
