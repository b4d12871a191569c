"""The session call in fill mode (the bounding-box gate) and with the RANSAC baseline, timed: ONE
submap_align_session call against the loop of submap_align_pools over the same robot pairs — the route a caller had before the
session call served these modes, and the baseline here —, on the same device-resident pools; roman_session_boxes_dev and
roman_session_gate_aabb_dev alone between two events; the RANSAC session against its own loop.

  python tools/gpu_session_aabb.py --out profiles/session_aabb/timing.json

Scale: the session of tools/gpu_session.py (R = 4 views of 10^4 segments with 768-d descriptors around a 1 km loop, 'roman',
'mean_semantic', the 10 blocks r <= s) with force_fill_submaps: slices of 40 segments, 20 shared with the next.  The pools are built
once per process, outside the timed region.  Each step runs in a process of its own under `timeout -k 10`: warm-up calls, then the
median; the parent starts the next step only after a clean end, compares the paths' results and writes the JSON.  No ratio is
promised: a session call slower than the loop is reported as such.

Beside the JSON the tool writes kernel_resources.txt: the cross-compiled register, LDS and scratch figures of k_session_boxes and of
the session gate's instantiations (tools/kernel_resources.py, no GPU needed: `--resources-only` writes this file alone), and fails
if one of them uses scratch."""
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

from gpu_session import D, same_results, summary             # noqa: E402  (the same dump and the same comparison)

LIMITS = dict(session=420, loop=420, kernels=240, ransac_session=420, ransac_loop=420)       # seconds per step


def setup(a, ransac=False):
    import torch
    from roman_amd import synth
    from roman_amd.align import RansacReg, SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import FillSubmapParams, MapTable, build_submap_pool, fill_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="ransac" if ransac else "roman", semantics_dim=D, force_fill_submaps=True, submap_radius=15.0, submap_max_size=40, submap_overlap=20,
                          submap_descriptor='mean_semantic', submap_descriptor_thresh=a.thresh, single_robot_lc_time_thresh=a.time_thresh)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=a.skip)
    roman = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); roman.set_context(ctx)
    reg = roman
    if ransac:
        reg = RansacReg(max_iteration=a.ransac_iter); reg.set_context(ctx)
    fp = FillSubmapParams.from_submap_align_params(p)
    segs, traj, times = synth.make_map(a.segments, D, seed=8100, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
    pools = []
    for r in range(a.robots):                                # the views of tools/gpu_session.py
        rng = np.random.default_rng(8200 + r)
        pick = np.sort(rng.permutation(len(segs))[:int(round((1.0 - 0.05 * r) * len(segs)))])
        mine = []
        for k in pick.tolist():
            q = copy.copy(segs[k])
            q.id = int(segs[k].id) + 10 ** 6 * r
            q.centroid = np.asarray(segs[k].centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(segs[k].centroid))
            mine.append(q)
        table = MapTable.from_segments(roman, mine)
        centers, slices = fill_centers(table, traj[40 * r:], times[40 * r:], fp)
        pools.append(build_submap_pool(roman, table, centers, fp, ctx=ctx, device=dev, fill=slices))
    blocks = [(r, s) for r in range(a.robots) for s in range(r, a.robots)]
    return torch, dev, stream, ctx, p, io, reg, pools, blocks


def step_path(a, which, ransac):
    from roman_amd.align import submap_align as sa
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a, ransac)
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
               loop_closures=int(sum(len(r.lc_edges["pairs"]) for r in res.values())),
               nearby=int(sum(int((~np.isnan(r.robots_nearby_mat)).sum()) for r in res.values())))
    np.savez(a.dump, **summary(res, blocks))
    ctx.close()
    return out


def step_kernels(a):
    """roman_session_boxes_dev and roman_session_gate_aabb_dev alone, each between two events on the context's stream."""
    from roman_amd.runtime import grid_gate_params, session_tables
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a)
    keep = [q.nonempty for q in pools]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tabs = session_tables([len(k) for k in keep], [(r, s, r == s) for r, s in blocks])
    dtab = [up(x) for x in tabs]
    pose = np.concatenate([q.centers.pose_flu[k] for q, k in zip(pools, keep)])
    pos, T_w, tm = up(pose[:, :3, 3]), up(pose.reshape(-1, 16)), up(np.concatenate([q.centers.time[k] for q, k in zip(pools, keep)]))
    desc = torch.cat([q.desc_dev[torch.from_numpy(k.astype(np.int64)).to(dev)] for q, k in zip(pools, keep)]).contiguous()
    pool = torch.cat([q.pool for q in pools], dim=0)
    base = np.concatenate([[0], np.cumsum([int(q.pool.shape[0]) for q in pools])])
    row0 = up(np.concatenate([base[r] + q.offsets()[0] for r, q in enumerate(pools)]).astype(np.int64))
    cnt = up(np.concatenate([q.offsets()[1] for q in pools]).astype(np.int32))
    S, B, nb = int(tabs[0][-1]), int(tabs[2][-1]), len(blocks)
    f64, i32 = torch.float64, torch.int32
    box = torch.empty((S, 6), dtype=f64, device=dev)
    o = [torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=f64, device=dev),
         torch.empty(16 * B, dtype=f64, device=dev), torch.empty(2 * B, dtype=i32, device=dev), torch.empty(16 * B, dtype=f64, device=dev),
         torch.empty(B, dtype=i32, device=dev), torch.zeros(nb + 1, dtype=i32, device=dev)]
    gp = grid_gate_params(None, a.skip, D, a.thresh, False, a.time_thresh)

    def timed(call):
        ms = []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            call()
            e1.record(stream)
            ctx.sync(); e1.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))
    boxes = timed(lambda: ctx.session_boxes_dev(S, int(pool.shape[1]), pool.data_ptr(), row0.data_ptr(), cnt.data_ptr(), T_w.data_ptr(), box.data_ptr()))
    gate = timed(lambda: ctx.session_gate_aabb_dev(gp, *tabs, *[x.data_ptr() for x in dtab], pos.data_ptr(), T_w.data_ptr(), *[x.data_ptr() for x in o],
                                                   box.data_ptr(), time_ptr=tm.data_ptr(), desc_ptr=desc.data_ptr()))
    out = dict(submaps=S, row_width=int(pool.shape[1]), rows=int(pool.shape[0]), blocks=nb, pairs=B, d=D, n_todo=int(o[8].cpu().numpy()[-1]),
               session_boxes=boxes, session_gate_aabb=gate)
    ctx.close()
    return out


RESOURCE_KERNELS = ("k_submap_boxes", "k_session_boxes", "k_session_gate<")


def write_resources(path):
    """The rows of tools/kernel_resources.py for k_session_boxes (beside k_submap_boxes, whose wave body it shares) and every
    instantiation of k_session_gate -> `path`.  -> False when a kernel spills (ScratchSize != 0)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True).stdout.splitlines()
    rows = [l for l in out[1:] if l.startswith(RESOURCE_KERNELS)]
    names = [l.split()[0] for l in rows]
    ok = bool(rows) and "k_session_boxes" in names and sum(n.startswith("k_session_gate<") for n in names) == 4 and all(l.split()[-3] == "0" for l in rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join([out[0]] + rows) + "\n\nFrom the library's own compile line for gfx950 (tools/kernel_resources.py); ScratchSize 0: no spills.\n"
                "k_session_gate<true> and <false> are the radius-mode kernels, <true, true> and <false, true> the bounding-box gate.\n")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=list(LIMITS), help="(internal) run one step in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference's default)")
    ap.add_argument("--skip", type=float, default=float("inf"), help="skip_distance")
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0, help="single_robot_lc_time_thresh of the self blocks")
    ap.add_argument("--ransac-iter", dest="ransac_iter", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_aabb", "timing.json"))
    ap.add_argument("--resources-only", dest="resources_only", action="store_true", help="write kernel_resources.txt beside --out and stop (no GPU)")
    ap.add_argument("--no-resources", dest="no_resources", action="store_true", help="leave kernel_resources.txt as it is")
    a = ap.parse_args()
    res_path = os.path.join(os.path.dirname(os.path.abspath(a.out)), "kernel_resources.txt")
    if a.resources_only:
        return 0 if write_resources(res_path) else 3
    if a.step:
        res = step_kernels(a) if a.step == "kernels" else step_path(a, "session" if a.step.endswith("session") else "loop", a.step.startswith("ransac"))
        print("STEP_RESULT " + json.dumps(res))
        return 0
    nb = a.robots * (a.robots + 1) // 2
    out = dict(scale=dict(robots=a.robots, blocks=nb, segments=a.segments, d=D, submap_descriptor="mean_semantic", force_fill_submaps=True, max_size=40, overlap=20,
                          thresh=a.thresh, reps=a.reps, warmup=a.warmup, ransac_iter=a.ransac_iter))
    names = dict(session="session_call", loop="loop_of_submap_align_pools", kernels="kernels_alone", ransac_session="ransac_session_call",
                 ransac_loop="ransac_loop_of_submap_align_pools")
    with tempfile.TemporaryDirectory() as td:
        for step in LIMITS:
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--dump", os.path.join(td, step + ".npz"),
                   "--robots", str(a.robots), "--segments", str(a.segments), "--reps", str(a.reps), "--warmup", str(a.warmup), "--thresh", str(a.thresh),
                   "--skip", str(a.skip), "--time-thresh", str(a.time_thresh), "--ransac-iter", str(a.ransac_iter)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
                print(f"step {step} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return 1
            out[names[step]] = json.loads(line[0][len("STEP_RESULT "):])
            print(step, line[0], flush=True)
        out["same_results"] = same_results(os.path.join(td, "session.npz"), os.path.join(td, "loop.npz"), nb)
        out["ransac_same_results"] = same_results(os.path.join(td, "ransac_session.npz"), os.path.join(td, "ransac_loop.npz"), nb)
    out["loop_over_session"] = out["loop_of_submap_align_pools"]["seconds_median"] / out["session_call"]["seconds_median"]
    out["ransac_loop_over_session"] = out["ransac_loop_of_submap_align_pools"]["seconds_median"] / out["ransac_session_call"]["seconds_median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not a.no_resources and not write_resources(res_path):
        return 3
    return 0 if out["same_results"] and out["ransac_same_results"] else 2


if __name__ == "__main__":
    sys.exit(main())
