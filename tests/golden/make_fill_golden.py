#!/usr/bin/env python3
"""Generate tests/golden/fill_golden.npz by running the REFERENCE'S OWN submaps_from_roman_map(force_fill_submaps=True)
([REF roman/map/map.py:264-295]) and aabb_intersects ([REF roman/utils.py:160-169]) over segments_as_global_points
([REF roman/map/map.py:133-139]) on the synthetic map of roman_amd.synth.make_map, under the stand-in modules
tests/golden/make_golden.py installs.  Re-run with:  python tests/golden/make_fill_golden.py

The reference is read only here, when the fixture is regenerated; tests read the committed .npz.  A case that
tests/_fill_boxes_oracle.borderline flags is REFUSED: the fixture only holds parameters for which the reference alone is
unambiguous (no box comparison with its two sides within 1e-9, no slice whose mean time is within 1e-9 of equidistant between two
trajectory times); the number of flags — zero — is stored with every case."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository root and tests/ on sys.path)
from make_submaps_golden import MapSegment  # noqa: E402

from roman_amd import synth  # noqa: E402

CASES = [("m12_o6", 12, 6), ("m8_o3", 8, 3), ("m40_o0", 40, 0), ("m200_o10", 200, 10)]     # name, max_size, overlap (the last: one slice, max_size > N)
N, D, N_POSES = 120, 16, 50


def build_map():
    segs, traj, times = synth.make_map(N, D, seed=8100, n_poses=N_POSES, dt=8.0)
    for s in segs:
        s.__class__ = MapSegment
    return segs, traj, times


def main():
    make_golden.install_reference_stubs()
    from roman.map.map import ROMANMap, SubmapParams as RefSubmapParams, submaps_from_roman_map
    from roman.utils import aabb_intersects
    from roman_amd.align.submaps import FillSubmapParams, MapTable, fill_centers
    from roman_amd.align import SubmapAlignParams
    import _fill_boxes_oracle as fo

    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    segs, traj, times = build_map()
    table = MapTable.from_segments(reg, segs)
    index_of = {s.id: k for k, s in enumerate(segs)}
    out = {"names": np.array([c[0] for c in CASES]), "feats": table.feats, "times": table.times, "ids": table.ids,
           "trajectory": np.array(traj), "traj_times": np.array(times)}
    for name, max_size, overlap in CASES:
        centers, slices = fill_centers(table, traj, times, FillSubmapParams(max_size=max_size, overlap=overlap))
        _, mean, _ = fo.fill_slices(table.times, times, max_size, overlap)
        mine = fo.fill_oracle(table.feats, centers.descs(), slices, max_size)
        pool = np.zeros((len(slices) * max_size, table.feats.shape[1]))
        for s, rows in enumerate(mine["rows"]):
            pool[s * max_size:s * max_size + len(rows)] = rows
        box = fo.boxes_oracle(pool, max_size, mine["count"], centers.pose_flu)
        flags = fo.borderline(box, box, mean, times)
        if flags:
            sys.exit(f"case {name}: borderline input, refusing to write it: {flags[:3]}")
        rmap = ROMANMap(segments=copy.deepcopy(segs), trajectory=[T.copy() for T in traj], times=np.array(times))
        ref = submaps_from_roman_map(rmap, RefSubmapParams(max_size=max_size, force_fill_submaps=True, overlap=overlap, object_center_ref='mean',
                                                           use_minimal_data=False, submap_descriptor='mean_semantic'))
        S = len(ref)
        pts = [sm.segments_as_global_points for sm in ref]
        out[f"{name}/max_size"] = max_size; out[f"{name}/overlap"] = overlap; out[f"{name}/S"] = S; out[f"{name}/n_borderline"] = len(flags)
        out[f"{name}/sm_time"] = np.array([sm.time for sm in ref], dtype=np.float64)
        out[f"{name}/sm_index"] = np.array([int(np.nonzero(np.asarray(times) == sm.time)[0][0]) for sm in ref], dtype=np.int64)
        out[f"{name}/sm_desc"] = np.array([sm.descriptor for sm in ref], dtype=np.float64).reshape(S, D)
        out[f"{name}/nearby"] = np.array([[bool(aabb_intersects(pts[i], pts[j])) for j in range(S)] for i in range(S)], dtype=bool).reshape(S, S)
        for q, sm in enumerate(ref):
            out[f"{name}/src_{q}"] = np.array([index_of[s.id] for s in sm.segments], dtype=np.int32)
            out[f"{name}/cen_{q}"] = np.array([s.center.reshape(-1) for s in sm.segments], dtype=np.float64).reshape(len(sm.segments), 3)
        print(f"  {name:10s} S={S} sizes={[len(sm.segments) for sm in ref]} nearby={int(out[f'{name}/nearby'].sum())}/{S * S} borderline={len(flags)}")
    path = os.path.join(HERE, "fill_golden.npz")
    np.savez_compressed(path, **out)
    print(f"fill_golden.npz written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    if not os.path.isdir(make_golden.REF):
        sys.exit("reference checkout not present: golden fixtures can only be regenerated where it exists")
    main()
