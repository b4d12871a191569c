"""Two maps to loop closures, end to end: the device-resident path (build_submap_pool x 2 + submap_align_pools) against the path
through host submaps (build_submap_pool x 2 + SubmapPool.to_submaps + submap_align_grid) on the same two synthetic maps, and the
gate's own device time (roman_grid_gate_dev between two events).

  python tools/gpu_pools_grid.py --out profiles/pools_grid/timing.json

Scale: two maps of 10^4 segments with 768-d descriptors around a 1 km loop, about 100 submap centres each (10 m apart, radius
15 m, at most 40 segments per submap), method 'roman', submap_descriptor 'mean_semantic'.  Each path runs in a process of its
own under `timeout -k 10`: 3 warm-up calls, then the median of 10; the parent starts the next step only after a clean end,
compares the two paths' results and writes the JSON.  No ratio is promised: the numbers are what they are."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 768
LIMITS = dict(pools=420, grid=600, gate=180)              # seconds per step


def setup(a):
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40,
                          submap_descriptor='mean_semantic', submap_descriptor_thresh=a.thresh)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=a.skip)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    maps = []
    for seed in (8100, 8100):                                  # the same place mapped twice: cross pairs have true matches
        segs, traj, times = synth.make_map(a.segments, D, seed=seed, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
        maps.append((segs, traj, times, MapTable.from_segments(reg, segs)))
    return torch, dev, stream, ctx, p, io, reg, params, maps


def build_pools(ctx, dev, reg, params, maps):
    from roman_amd.align.submaps import build_submap_pool, submap_centers
    return [build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=ctx, device=dev) for (_, traj, times, table) in maps]


def summary(res):
    n = np.nan_to_num(res.clipper_num_associations, nan=-1.0)
    return dict(n=n, nearby=np.nan_to_num(res.robots_nearby_mat, nan=-1.0), pairs=np.asarray(res.lc_edges["pairs"]),
                t=np.asarray(res.lc_edges["t"]), q=np.asarray(res.lc_edges["q"]), That=np.nan_to_num(res.T_ij_hat_mat, nan=0.0))


def step_path(a, which):
    from roman_amd.align import submap_align as sa
    torch, dev, stream, ctx, p, io, reg, params, maps = setup(a)
    phases = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pools = build_pools(ctx, dev, reg, params, maps)
        t1 = time.perf_counter()
        if which == "pools":
            res = sa.submap_align_pools(p, pools, io, registration=reg)
            t2 = t1
        else:
            subs = [q.to_submaps(m[0]) for q, m in zip(pools, maps)]
            t2 = time.perf_counter()
            res = sa.submap_align_grid(p, subs, io, registration=reg)
        t3 = time.perf_counter()
        if rep >= a.warmup:
            phases.append(dict(build_pools=t1 - t0, to_submaps=t2 - t1, align=t3 - t2, total=t3 - t0))
    out = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    out.update(submaps=[int(len(q.nonempty)) for q in pools], registered=len(res.timing_list), loop_closures=int(len(res.lc_edges["pairs"])))
    np.savez(a.dump, **summary(res))
    ctx.close()
    return out


def step_gate(a):
    from roman_amd.runtime import grid_gate_params
    torch, dev, stream, ctx, p, io, reg, params, maps = setup(a)
    pools = build_pools(ctx, dev, reg, params, maps)
    keep = [q.nonempty for q in pools]
    n0, n1 = len(keep[0]), len(keep[1])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    side = [dict(pos=up(q.centers.pose_flu[k][:, :3, 3]), T_w=up(q.centers.pose_flu[k].reshape(-1, 16)), time=up(q.centers.time[k]),
                 desc=q.desc_dev[torch.from_numpy(k.astype(np.int64)).to(dev)].contiguous()) for q, k in zip(pools, keep)]
    B = n0 * n1
    f64, i32 = torch.float64, torch.int32
    o = dict(dist=torch.empty(B, dtype=f64, device=dev), flags=torch.empty(B, dtype=i32, device=dev), yaw=torch.empty(B, dtype=f64, device=dev),
             sim=torch.empty(B, dtype=f64, device=dev), T_ij=torch.empty(16 * B, dtype=f64, device=dev), pairs=torch.empty(2 * B, dtype=i32, device=dev),
             T_ref=torch.empty(16 * B, dtype=f64, device=dev), enable=torch.empty(B, dtype=i32, device=dev), n=torch.zeros(1, dtype=i32, device=dev))
    gp = grid_gate_params(15.0, a.skip, D, a.thresh, False, 0.0)
    ms = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        ctx.grid_gate_dev(gp, n0, n1, side[0]["pos"].data_ptr(), side[0]["T_w"].data_ptr(), side[1]["pos"].data_ptr(), side[1]["T_w"].data_ptr(),
                          o["dist"].data_ptr(), o["flags"].data_ptr(), o["yaw"].data_ptr(), o["sim"].data_ptr(), o["T_ij"].data_ptr(),
                          o["pairs"].data_ptr(), o["T_ref"].data_ptr(), o["enable"].data_ptr(), o["n"].data_ptr(),
                          time0_ptr=side[0]["time"].data_ptr(), time1_ptr=side[1]["time"].data_ptr(),
                          desc0_ptr=side[0]["desc"].data_ptr(), desc1_ptr=side[1]["desc"].data_ptr())
        e1.record(stream)
        ctx.sync(); e1.synchronize()
        if rep >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    out = dict(grid=[n0, n1], d=D, n_todo=int(o["n"].cpu().numpy()[0]), gate_ms_median=float(np.median(ms)), gate_ms_min=float(np.min(ms)))
    ctx.close()
    return out


def same_results(fa, fb):
    A, B = np.load(fa), np.load(fb)
    exact = all(np.array_equal(A[k], B[k]) for k in ("n", "nearby", "pairs"))
    tol = all(A[k].shape == B[k].shape and np.allclose(A[k], B[k], rtol=0, atol=1e-12) for k in ("t", "q", "That"))
    return bool(exact and tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=["pools", "grid", "gate"], help="(internal) run one step in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference's default)")
    ap.add_argument("--skip", type=float, default=float("inf"), help="skip_distance")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pools_grid", "timing.json"))
    a = ap.parse_args()
    if a.step:
        res = step_gate(a) if a.step == "gate" else step_path(a, a.step)
        print("STEP_RESULT " + json.dumps(res))
        return 0
    out = dict(scale=dict(segments=a.segments, d=D, method="roman", submap_descriptor="mean_semantic", thresh=a.thresh, reps=a.reps, warmup=a.warmup))
    with tempfile.TemporaryDirectory() as td:
        for step in ("pools", "grid", "gate"):
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--dump", os.path.join(td, step + ".npz"),
                   "--segments", str(a.segments), "--reps", str(a.reps), "--warmup", str(a.warmup), "--thresh", str(a.thresh), "--skip", str(a.skip)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
                print(f"step {step} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return 1
            out[{"pools": "device_resident_path", "grid": "host_submaps_path", "gate": "gate_alone"}[step]] = json.loads(line[0][len("STEP_RESULT "):])
            print(step, line[0])
        out["same_results"] = same_results(os.path.join(td, "pools.npz"), os.path.join(td, "grid.npz"))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if out["same_results"] else 2


if __name__ == "__main__":
    sys.exit(main())
