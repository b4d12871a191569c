"""A session of R robots to loop closures: ONE submap_align_session call against the loop of submap_align_pools over the same robot
pairs (the loop a caller writes without the session call), on the same device-resident pools, and the session gate's own device
time (roman_session_gate_dev between two events).

  python tools/gpu_session.py --out profiles/session/timing.json

Scale: R = 4 maps of the same place (each robot its own view of it: 100, 95, 90, 85 % of 10^4 segments, centres a few cm off, the
drive opened later) with 768-d descriptors around a 1 km loop, about 100 submap centres each (10 m apart, radius
15 m, at most 40 segments per submap), method 'roman', submap_descriptor 'mean_semantic': the 10 blocks r <= s, the 4 self blocks
with the shared-segment removal.  The pools are built once per process, outside the timed region.  Each path runs in a process of
its own under `timeout -k 10`: 3 warm-up calls, then the median of 10; the parent starts the next step only after a clean end,
compares the two paths' results and writes the JSON.  No ratio is promised: the numbers are what they are."""
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

D = 768
LIMITS = dict(session=420, loop=420, gate=240)            # seconds per step


def setup(a):
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
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
    pools = []
    for r in range(a.robots):
        # the same place mapped by every robot (cross pairs have true matches), each with its own view of it: 100, 95, 90, ... % of
        # the segments, every centre a few cm off, ids of its own, the drive opened 40 poses later per robot
        rng = np.random.default_rng(8200 + r)
        pick = np.sort(rng.permutation(len(segs))[:int(round((1.0 - 0.05 * r) * len(segs)))])
        mine = []
        for k in pick.tolist():
            q = copy.copy(segs[k])
            q.id = int(segs[k].id) + 10 ** 6 * r
            q.centroid = np.asarray(segs[k].centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(segs[k].centroid))
            mine.append(q)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, mine), submap_centers(traj[40 * r:], times[40 * r:], params), params, ctx=ctx, device=dev))
    blocks = [(r, s) for r in range(a.robots) for s in range(r, a.robots)]
    return torch, dev, stream, ctx, p, io, reg, pools, blocks


def summary(results, blocks):
    out = {}
    for b, key in enumerate(blocks):
        res = results[key]
        out[f"n{b}"] = np.nan_to_num(res.clipper_num_associations, nan=-1.0); out[f"nearby{b}"] = np.nan_to_num(res.robots_nearby_mat, nan=-1.0)
        out[f"pairs{b}"] = np.asarray(res.lc_edges["pairs"]); out[f"t{b}"] = np.asarray(res.lc_edges["t"]); out[f"q{b}"] = np.asarray(res.lc_edges["q"])
        out[f"That{b}"] = np.nan_to_num(res.T_ij_hat_mat, nan=0.0)
    return out


def step_path(a, which):
    from roman_amd.align import submap_align as sa
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a)
    secs = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if which == "session":
            res = sa.submap_align_session(p, pools, blocks, io, registration=reg)
        else:
            res = {}
            for r, s in blocks:
                q = copy.copy(p); q.single_robot_lc = (r == s)
                res[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
        torch.cuda.synchronize(dev)
        if rep >= a.warmup:
            secs.append(time.perf_counter() - t0)
    out = dict(seconds_median=float(np.median(secs)), seconds_min=float(np.min(secs)), seconds_max=float(np.max(secs)), seconds=[float(x) for x in secs], blocks=len(blocks),
               submaps=[int(len(q.nonempty)) for q in pools], registered=int(sum(len(r.timing_list) for r in res.values())),
               loop_closures=int(sum(len(r.lc_edges["pairs"]) for r in res.values())))
    np.savez(a.dump, **summary(res, blocks))
    ctx.close()
    return out


def step_gate(a):
    from roman_amd.runtime import grid_gate_params, session_tables
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a)
    keep = [q.nonempty for q in pools]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tabs = session_tables([len(k) for k in keep], [(r, s, r == s) for r, s in blocks])
    dtab = [up(x) for x in tabs]
    pose = np.concatenate([q.centers.pose_flu[k] for q, k in zip(pools, keep)])
    pos, T_w, tm = up(pose[:, :3, 3]), up(pose.reshape(-1, 16)), up(np.concatenate([q.centers.time[k] for q, k in zip(pools, keep)]))
    desc = torch.cat([q.desc_dev[torch.from_numpy(k.astype(np.int64)).to(dev)] for q, k in zip(pools, keep)]).contiguous()
    B, nb = int(tabs[2][-1]), len(blocks)
    f64, i32 = torch.float64, torch.int32
    o = [torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=f64, device=dev),
         torch.empty(16 * B, dtype=f64, device=dev), torch.empty(2 * B, dtype=i32, device=dev), torch.empty(16 * B, dtype=f64, device=dev),
         torch.empty(B, dtype=i32, device=dev), torch.zeros(nb + 1, dtype=i32, device=dev)]
    gp = grid_gate_params(15.0, a.skip, D, a.thresh, False, a.time_thresh)
    ms = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        ctx.session_gate_dev(gp, *tabs, *[x.data_ptr() for x in dtab], pos.data_ptr(), T_w.data_ptr(), *[x.data_ptr() for x in o],
                             time_ptr=tm.data_ptr(), desc_ptr=desc.data_ptr())
        e1.record(stream)
        ctx.sync(); e1.synchronize()
        if rep >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    out = dict(blocks=nb, pairs=B, d=D, n_todo=int(o[8].cpu().numpy()[-1]), gate_ms_median=float(np.median(ms)), gate_ms_min=float(np.min(ms)))
    ctx.close()
    return out


def same_results(fa, fb, nb):
    A, B = np.load(fa), np.load(fb)
    exact = all(np.array_equal(A[f"{k}{b}"], B[f"{k}{b}"]) for b in range(nb) for k in ("n", "nearby", "pairs"))
    tol = all(A[f"{k}{b}"].shape == B[f"{k}{b}"].shape and np.allclose(A[f"{k}{b}"], B[f"{k}{b}"], rtol=0, atol=1e-12) for b in range(nb) for k in ("t", "q", "That"))
    return bool(exact and tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=["session", "loop", "gate"], help="(internal) run one step in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference's default)")
    ap.add_argument("--skip", type=float, default=float("inf"), help="skip_distance")
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0, help="single_robot_lc_time_thresh of the self blocks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session", "timing.json"))
    a = ap.parse_args()
    if a.step:
        res = step_gate(a) if a.step == "gate" else step_path(a, a.step)
        print("STEP_RESULT " + json.dumps(res))
        return 0
    nb = a.robots * (a.robots + 1) // 2
    out = dict(scale=dict(robots=a.robots, blocks=nb, segments=a.segments, d=D, method="roman", submap_descriptor="mean_semantic", thresh=a.thresh,
                          reps=a.reps, warmup=a.warmup))
    names = dict(session="session_call", loop="loop_of_submap_align_pools", gate="session_gate_alone")
    with tempfile.TemporaryDirectory() as td:
        for step in ("session", "loop", "gate"):
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--dump", os.path.join(td, step + ".npz"),
                   "--robots", str(a.robots), "--segments", str(a.segments), "--reps", str(a.reps), "--warmup", str(a.warmup), "--thresh", str(a.thresh),
                   "--skip", str(a.skip), "--time-thresh", str(a.time_thresh)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
                print(f"step {step} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return 1
            out[names[step]] = json.loads(line[0][len("STEP_RESULT "):])
            print(step, line[0], flush=True)
        out["same_results"] = same_results(os.path.join(td, "session.npz"), os.path.join(td, "loop.npz"), nb)
    out["loop_over_session"] = out["loop_of_submap_align_pools"]["seconds_median"] / out["session_call"]["seconds_median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if out["same_results"] else 2


if __name__ == "__main__":
    sys.exit(main())
