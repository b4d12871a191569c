"""A session of R robots from maps to loop closures with the pools built INSIDE the timed region: build_session_pools (one
roman_session_submaps_dev call, one allocation) + submap_align_session against the way before it — build_submap_pool per robot +
submap_align_session, which concatenates the four pools — and the build alone for both ways, between two events.

  python tools/gpu_session_submaps.py --out profiles/session_submaps/timing.json

Scale: the four maps of tools/gpu_session.py (the same place, 100, 95, 90, 85 % of 10^4 segments with 768-d descriptors, about 100
submap centres each, at most 40 segments per submap, method 'roman', 'mean_semantic', the 10 blocks r <= s).  The map tables and
the centres are made once per process, outside the timed region; what is timed starts at the tables in host memory.  Each way runs
in a process of its own under `timeout -k 10`: 3 warm-up calls, then the median of 10, every sample kept; the parent starts the next
step only after a clean end, compares the two ways' results per block (counts, nearby matrix and accepted pairs exactly, poses and
edges to 1e-12) and writes the JSON.  No ratio is promised: the numbers are what they are."""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D = 768
LIMIT = 540                                              # seconds per step


def setup(a):
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, submap_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40,
                          submap_descriptor='mean_semantic', submap_descriptor_thresh=a.thresh, single_robot_lc_time_thresh=a.time_thresh)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=a.skip)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    segs, traj, times = synth.make_map(a.segments, D, seed=8100, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
    tables, centers = [], []
    for r in range(a.robots):                            # (the four views of tools/gpu_session.py)
        rng = np.random.default_rng(8200 + r)
        pick = np.sort(rng.permutation(len(segs))[:int(round((1.0 - 0.05 * r) * len(segs)))])
        mine = []
        for k in pick.tolist():
            q = copy.copy(segs[k])
            q.id = int(segs[k].id) + 10 ** 6 * r
            q.centroid = np.asarray(segs[k].centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(segs[k].centroid))
            mine.append(q)
        tables.append(MapTable.from_segments(reg, mine)); centers.append(submap_centers(traj[40 * r:], times[40 * r:], params))
    blocks = [(r, s) for r in range(a.robots) for s in range(r, a.robots)]
    return torch, dev, stream, ctx, p, io, reg, params, tables, centers, blocks


def step_way(a, which):
    from gpu_session import summary
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import build_session_pools, build_submap_pool
    torch, dev, stream, ctx, p, io, reg, params, tables, centers, blocks = setup(a)

    def build():
        if which == "session":
            return build_session_pools(reg, tables, centers, params, ctx=ctx, device=dev)
        return [build_submap_pool(reg, t, c, params, ctx=ctx, device=dev) for t, c in zip(tables, centers)]
    secs, build_ms = [], []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pools = build()
        res = sa.submap_align_session(p, pools, blocks, io, registration=reg)
        torch.cuda.synchronize(dev)
        if rep >= a.warmup:
            secs.append(time.perf_counter() - t0)
    for rep in range(a.warmup + a.reps):                 # the build alone, uploads and read-backs included, between two events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(stream)
        pools = build()
        e1.record(stream)
        e1.synchronize()
        if rep >= a.warmup:
            build_ms.append(e0.elapsed_time(e1))
    out = dict(seconds_median=float(np.median(secs)), seconds_min=float(np.min(secs)), seconds_max=float(np.max(secs)), seconds=[float(x) for x in secs],
               build_ms_median=float(np.median(build_ms)), build_ms_min=float(np.min(build_ms)), build_ms=[float(x) for x in build_ms],
               segments=[len(t) for t in tables], submaps=[int(len(q.nonempty)) for q in pools], pool_rows=[int(q.pool.shape[0]) for q in pools],
               registered=int(sum(len(r.timing_list) for r in res.values())), loop_closures=int(sum(len(r.lc_edges["pairs"]) for r in res.values())))
    np.savez(a.dump, **summary(res, blocks))
    ctx.close()
    return out


def main():
    from gpu_session import same_results
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=["session", "per_robot"], help="(internal) run one way in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference's default)")
    ap.add_argument("--skip", type=float, default=float("inf"), help="skip_distance")
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0, help="single_robot_lc_time_thresh of the self blocks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_submaps", "timing.json"))
    a = ap.parse_args()
    if a.step:
        print("STEP_RESULT " + json.dumps(step_way(a, a.step)))
        return 0
    nb = a.robots * (a.robots + 1) // 2
    out = dict(scale=dict(robots=a.robots, blocks=nb, segments=a.segments, d=D, method="roman", submap_descriptor="mean_semantic", thresh=a.thresh,
                          reps=a.reps, warmup=a.warmup))
    names = dict(session="build_session_pools_then_session", per_robot="build_submap_pool_per_robot_then_session")
    with tempfile.TemporaryDirectory() as td:
        for step in ("session", "per_robot"):
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", step, "--dump", os.path.join(td, step + ".npz"),
                   "--robots", str(a.robots), "--segments", str(a.segments), "--reps", str(a.reps), "--warmup", str(a.warmup), "--thresh", str(a.thresh),
                   "--skip", str(a.skip), "--time-thresh", str(a.time_thresh)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
                print(f"step {step} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return 1
            out[names[step]] = json.loads(line[0][len("STEP_RESULT "):])
            print(step, line[0], flush=True)
        out["same_results"] = same_results(os.path.join(td, "session.npz"), os.path.join(td, "per_robot.npz"), nb)
    out["per_robot_over_session"] = out[names["per_robot"]]["seconds_median"] / out[names["session"]]["seconds_median"]
    out["build_per_robot_over_session"] = out[names["per_robot"]]["build_ms_median"] / out[names["session"]]["build_ms_median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if out["same_results"] else 2


if __name__ == "__main__":
    sys.exit(main())
