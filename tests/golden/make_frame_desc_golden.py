#!/usr/bin/env python3
"""Generate tests/golden/frame_desc_golden.npz by running the REFERENCE'S OWN submaps_from_roman_map with the three
frame-descriptor modes ([REF roman/map/map.py:210-242]: mean_frame_descriptor, stacked_frame_descriptors with and without
frame_descriptor_dist) and its Submap.similarity [REF :144-162] over the grid of the map's submaps under one seeded table of frame
descriptors against the same submaps under a second table (two robots that drove the same path), on the synthetic map of
roman_amd.synth.make_map, under the stand-in modules tests/golden/make_golden.py
installs.  Re-run with:  python tests/golden/make_frame_desc_golden.py

The reference is read only here, when the fixture is regenerated; tests read the committed .npz.  A case that
tests/_frame_desc_oracle.borderline (or tests/_submaps_oracle.borderline, for the submaps underneath) flags is REFUSED."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository root and tests/ on sys.path)
from make_submaps_golden import MapSegment  # noqa: E402

from roman_amd import synth  # noqa: E402

N, D, N_POSES = 300, 16, 50          # 50 frames over 1.3 laps of a 25 m circle: about 12 centres 10 m apart, frames about 4 m apart
KW = dict(max_size=40, radius=15.0, distance=10.0, time_threshold=40.0, pruning_method='distance')
CASES = [
    # name, submap_descriptor, frame_descriptor_dist
    ("mean", 'mean_frame_descriptor', None),
    ("stacked_all", 'stacked_frame_descriptors', None),
    ("stacked_10m", 'stacked_frame_descriptors', 10.0),
]
SEED = 4242


def build_map():
    import _frame_desc_oracle as fo
    segs, traj, times = synth.make_map(N, D, seed=8100, n_poses=N_POSES, dt=8.0)
    for s in segs:
        s.__class__ = MapSegment
    desc = [fo.frame_descriptors(np.random.default_rng(SEED + r), N_POSES, D) for r in range(2)]
    return segs, traj, times, desc


def main():
    make_golden.install_reference_stubs()
    from roman.map.map import ROMANMap, Submap as RefSubmap, SubmapParams as RefSubmapParams, submaps_from_roman_map
    from roman_amd.align.submaps import MapTable, SubmapParams, submap_centers
    from roman_amd.align import SubmapAlignParams
    import _frame_desc_oracle as fo
    import _submaps_oracle as so

    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    segs, traj, times, desc = build_map()
    table = MapTable.from_segments(reg, segs)
    centers = submap_centers(traj, times, SubmapParams(**KW))
    flags = so.borderline(table.feats, table.times, centers.descs(), max_size=KW["max_size"], prune_by_time=False, radius=KW["radius"])
    if flags:
        sys.exit(f"borderline submaps, refusing to write: {flags[:3]}")
    index_of = {s.id: k for k, s in enumerate(segs)}
    pos = np.array([T[:3, 3] for T in traj])
    out = {"names": np.array([c[0] for c in CASES]), "feats": table.feats, "times": table.times, "ids": table.ids,
           "trajectory": np.array(traj), "traj_times": np.array(times), "frame_desc": desc[0], "frame_desc_b": desc[1],
           "kw": repr({k: (None if v is None else (float(v) if isinstance(v, float) else v)) for k, v in KW.items()})}
    for name, mode, dist in CASES:
        both = []
        for r in range(2):
            rmap = ROMANMap(segments=copy.deepcopy(segs), trajectory=[T.copy() for T in traj], times=np.array(times),
                            descriptors=[row.copy() for row in desc[r]])
            both.append(submaps_from_roman_map(rmap, RefSubmapParams(**KW, object_center_ref='mean', use_minimal_data=False, submap_descriptor=mode,
                                                                     frame_descriptor_dist=dist, force_fill_submaps=False)))
        ref, ref_b = both
        src = [np.array([index_of[s.id] for s in sm.segments], dtype=np.int32) for sm in ref]
        cap = KW["max_size"]
        count = np.array([len(x) for x in src], dtype=np.int32)
        src_pad = np.full((len(ref), cap), -1, np.int32)
        for q, x in enumerate(src):
            src_pad[q, :len(x)] = x
        flags = fo.borderline(count, src_pad, table.times, times, pos, dist if mode == 'stacked_frame_descriptors' else None)
        if flags:
            sys.exit(f"case {name}: borderline input, refusing to write it: {flags[:3]}")
        # which frames the reference took: every frame descriptor of the seeded table is distinct, so a row identifies its frame
        sel = []
        for sm in ref:
            if mode == 'mean_frame_descriptor':
                lo, hi = sm.first_seen, sm.last_seen
                sel.append(np.nonzero((np.array(times) >= lo) & (np.array(times) <= hi))[0].astype(np.int64))
            else:
                rows = np.asarray(sm.descriptor).reshape(-1, D)
                idx = [int(np.nonzero((desc[0] == r).all(axis=1))[0][0]) for r in rows]
                sel.append(np.array(idx, dtype=np.int64))
        flags = fo.borderline_sim(desc[0], sel, desc[1], sel)
        if flags:
            sys.exit(f"case {name}: borderline descriptors, refusing to write: {flags}")
        sim = np.array([[float(RefSubmap.similarity(a, b)) for b in ref_b] for a in ref], dtype=np.float64)
        out[f"{name}/mode"] = mode
        out[f"{name}/frame_descriptor_dist"] = np.float64(np.nan if dist is None else dist)
        out[f"{name}/n_submaps"] = len(ref)
        out[f"{name}/sm_id"] = np.array([sm.id for sm in ref], dtype=np.int64)
        out[f"{name}/mean"] = (np.array([sm.descriptor for sm in ref], dtype=np.float64).reshape(len(ref), D) if mode == 'mean_frame_descriptor'
                               else np.zeros((0, D)))
        out[f"{name}/mean_b"] = (np.array([sm.descriptor for sm in ref_b], dtype=np.float64).reshape(len(ref_b), D) if mode == 'mean_frame_descriptor'
                                 else np.zeros((0, D)))
        out[f"{name}/sim"] = sim
        for q in range(len(ref)):
            out[f"{name}/src_{q}"] = src[q]; out[f"{name}/sel_{q}"] = sel[q]
        print(f"  {name:12s} submaps={len(ref)} frames per submap={[len(x) for x in sel]} sim in [{sim.min():.3f}, {sim.max():.3f}]")
    path = os.path.join(HERE, "frame_desc_golden.npz")
    np.savez_compressed(path, **out)
    print(f"frame_desc_golden.npz written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    if not os.path.isdir(make_golden.REF):
        sys.exit("reference checkout not present: golden fixtures can only be regenerated where it exists")
    main()
