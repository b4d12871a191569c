"""Wall time of submap_align() (the per-pair host loops around one batched call) and of submap_align_grid() (pass 1 vectorised,
pass 2 and the loop-closure edges on the device) on the same synthetic grid, phase by phase.

  python tools/gpu_submap_align_grid.py --scale demo --grid 16 --out profiles/submap_align_grid_demo_16.json

Scales: `demo` (submaps of 20-40 objects, 768-d descriptors) and `config3` (n = m = 200, d = 512); method 'roman'.  The two
functions run alternately in one process, `--reps` times each (after one untimed warm-up each); medians are reported.  Phases:
pass 1 (everything before the device call, packing included), the device call, pass 2 / record unpacking, loop_closure_edges.
The split comes from timing the injected `compute` and the function as a whole."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roman_amd import synth                                   # noqa: E402
from roman_amd.align import SubmapAlignParams, batch as rb    # noqa: E402
from roman_amd.align import submap_align as sa                # noqa: E402


def make_grid(scale, S, seed=0):
    rng = np.random.default_rng(seed)
    d = 768 if scale == "demo" else 512
    # both robots see the same landmarks (one call of the generator), each submap in its own frame
    n = 40 if scale == "demo" else 200
    objs, poses = synth.make_submap_grid(2 * S, n=n, d=d, seed0=5000, overlap=0.6)
    if scale == "demo":                                         # 20-40 objects: every submap loses a random part of its 40
        objs = [[o[q] for q in sorted(rng.choice(n, size=int(rng.integers(20, 41)), replace=False))] for o in objs]
    submaps = [[], []]
    for r in range(2):
        for k in range(S):
            tilt = synth.yaw_transform(0.0, [0, 0, 0], roll=rng.normal(0, 0.02), pitch=rng.normal(0, 0.02))
            submaps[r].append(sa.Submap(id=k, time=1000.0 * r + 20.0 * k, segments=objs[S * r + k], pose_flu=poses[S * r + k] @ tilt))
    return submaps, d


def timed(fn, params, io, reg, submaps, device_compute):
    """-> dict of phase seconds for one run on a deep copy of the submaps."""
    subs = copy.deepcopy(submaps)
    inner = {}

    def compute(*a):
        t0 = time.perf_counter()
        out = device_compute(*a)
        inner["t0"], inner["t1"] = t0, time.perf_counter()
        return out
    t_start = time.perf_counter()
    res = fn(params, subs, io, registration=reg, compute=compute)
    t_end = time.perf_counter()
    edges = sa.loop_closure_edges(res, subs)
    t_edges = time.perf_counter()
    return dict(pass1=inner["t0"] - t_start, device_call=inner["t1"] - inner["t0"], pass2=t_end - inner["t1"],
                loop_closure_edges=t_edges - t_end, total=t_edges - t_start, n_edges=len(edges),
                n_pairs=int(np.count_nonzero(~np.isnan(res.T_ij_hat_mat[:, :, 0, 0]) | (res.clipper_num_associations == 0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=["demo", "config3"], default="demo")
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    submaps, d = make_grid(a.scale, a.grid)
    params = SubmapAlignParams(method="roman", semantics_dim=d, submap_radius=1e3)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = params.get_object_registration()
    legs = {"submap_align": (sa.submap_align, rb.run_batch), "submap_align_grid": (sa.submap_align_grid, rb.run_lc_batch)}
    runs = {k: [] for k in legs}
    for rep in range(a.reps + 1):                               # alternating; repetition 0 warms both up and is dropped
        for name, (fn, dc) in legs.items():
            t = timed(fn, params, io, reg, submaps, dc)
            if rep:
                runs[name].append(t)
    out = dict(scale=a.scale, grid=a.grid, pairs=a.grid * a.grid, reps=a.reps, method="roman", d=d)
    for name in legs:
        out[name] = {k: float(np.median([r[k] for r in runs[name]])) for k in ("pass1", "device_call", "pass2", "loop_closure_edges", "total")}
        out[name]["n_edges"] = runs[name][0]["n_edges"]
    out["speedup_total"] = out["submap_align"]["total"] / out["submap_align_grid"]["total"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
