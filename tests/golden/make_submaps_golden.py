#!/usr/bin/env python3
"""Generate tests/golden/submaps_golden.npz by running the REFERENCE'S OWN submaps_from_roman_map
([REF roman/map/map.py:244-357], radius mode) over the synthetic map of roman_amd.synth.make_map, under the stand-in modules
tests/golden/make_golden.py installs (robotdatapy, the segment classes).  Re-run with:  python tests/golden/make_submaps_golden.py

The reference is read only here, when the fixture is regenerated; tests read the committed .npz.  The map's segments are
SyntheticSegments with the three methods the reference's loop calls on a segment (set_center_ref, transform, reference_time),
written for this generator.  A case that tests/_submaps_oracle.borderline flags is REFUSED: the fixture only holds parameters
for which the reference alone is unambiguous (no radius / time test and no two keys within 1e-9 of a decision)."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository root and tests/ on sys.path)

from roman_amd import synth  # noqa: E402

CASES = [
    # name, SubmapParams kwargs of the reference, map variant
    ("distance", dict(max_size=40, radius=15.0, distance=10.0, time_threshold=np.inf, pruning_method='distance'), "loop"),
    ("time", dict(max_size=40, radius=15.0, distance=10.0, time_threshold=np.inf, pruning_method='time'), "loop"),
    ("no_radius_50s", dict(max_size=40, radius=None, distance=10.0, time_threshold=50.0, pruning_method='distance'), "loop"),
    ("no_max_size", dict(max_size=None, radius=15.0, distance=10.0, time_threshold=np.inf, pruning_method='distance'), "loop"),
    ("time_50s_small", dict(max_size=20, radius=15.0, distance=10.0, time_threshold=50.0, pruning_method='time'), "loop"),
    ("first_empty", dict(max_size=40, radius=15.0, distance=10.0, time_threshold=np.inf, pruning_method='distance'), "remote_start"),
]
N, D, N_POSES = 300, 16, 50          # 50 poses over 1.3 laps of a 25 m circle: about 12 centres 10 m apart


class MapSegment(synth.SyntheticSegment):
    """What the reference's loop calls on a segment, for the synthetic record."""

    def set_center_ref(self, ref):
        assert ref in ('bottom_middle', 'mean')

    def transform(self, T):
        self.centroid = T[:3, :3] @ self.centroid + T[:3, 3:4]

    def reference_time(self):
        return (self.first_seen + self.last_seen) / 2.0


def build_map(variant):
    segs, traj, times = synth.make_map(N, D, seed=8100, n_poses=N_POSES, dt=8.0)
    for s in segs:
        s.__class__ = MapSegment
    if variant == "remote_start":                                  # the first pose far from every segment: its submap stays empty
        far = traj[0].copy(); far[:3, 3] += np.array([300.0, 0.0, 0.0])
        traj = [far] + traj; times = np.concatenate([[times[0] - 8.0], times])
    return segs, traj, times


def main():
    make_golden.install_reference_stubs()
    from roman.map.map import ROMANMap, SubmapParams as RefSubmapParams, submaps_from_roman_map
    from roman_amd.align.submaps import MapTable, SubmapParams, submap_centers
    from roman_amd.align import SubmapAlignParams
    import _submaps_oracle as so

    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    out = {"names": np.array([c[0] for c in CASES])}
    for name, kw, variant in CASES:
        segs, traj, times = build_map(variant)
        table = MapTable.from_segments(reg, segs)
        mine = SubmapParams(**kw, submap_descriptor='mean_semantic')
        centers = submap_centers(traj, times, mine)
        flags = so.borderline(table.feats, table.times, centers.descs(), max_size=kw["max_size"],
                              prune_by_time=kw["pruning_method"] == 'time', radius=kw["radius"])
        if flags:
            sys.exit(f"case {name}: borderline input, refusing to write it: {flags[:3]}")
        rmap = ROMANMap(segments=copy.deepcopy(segs), trajectory=[T.copy() for T in traj], times=np.array(times))
        ref = submaps_from_roman_map(rmap, RefSubmapParams(**kw, object_center_ref='mean', use_minimal_data=False,
                                                           submap_descriptor='mean_semantic', force_fill_submaps=False))
        index_of = {s.id: k for k, s in enumerate(segs)}
        out[f"{name}/kw"] = repr({k: (None if v is None else (float(v) if isinstance(v, float) else v)) for k, v in kw.items()})
        out[f"{name}/variant"] = variant
        if "feats" in out:                                         # one segment table for every case; a trajectory per variant
            assert np.array_equal(out["feats"], table.feats) and np.array_equal(out["times"], table.times)
        out["feats"] = table.feats; out["times"] = table.times; out["ids"] = table.ids
        out[f"trajectory/{variant}"] = np.array(traj); out[f"traj_times/{variant}"] = np.array(times)
        out[f"{name}/n_centers"] = len(centers)
        out[f"{name}/sm_id"] = np.array([sm.id for sm in ref], dtype=np.int64)
        out[f"{name}/sm_time"] = np.array([sm.time for sm in ref], dtype=np.float64)
        out[f"{name}/sm_pose_flu"] = np.array([sm.pose_flu for sm in ref], dtype=np.float64).reshape(len(ref), 4, 4)
        out[f"{name}/sm_desc"] = np.array([sm.descriptor for sm in ref], dtype=np.float64).reshape(len(ref), D)
        for q, sm in enumerate(ref):
            out[f"{name}/src_{q}"] = np.array([index_of[s.id] for s in sm.segments], dtype=np.int32)
            out[f"{name}/cen_{q}"] = np.array([s.center.reshape(-1) for s in sm.segments], dtype=np.float64).reshape(len(sm.segments), 3)
        print(f"  {name:16s} centres={len(centers)} kept={len(ref)} sizes={[len(sm.segments) for sm in ref]}")
    path = os.path.join(HERE, "submaps_golden.npz")
    np.savez_compressed(path, **out)
    print(f"submaps_golden.npz written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    if not os.path.isdir(make_golden.REF):
        sys.exit("reference checkout not present: golden fixtures can only be regenerated where it exists")
    main()
