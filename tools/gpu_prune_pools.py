#!/usr/bin/env python3
"""method='clipper+prune' over device-resident pools.  Not a test and not bench.py.

    python tools/gpu_prune_pools.py [--out profiles/prune_pools] [--reps 10] [--warmup 3]

Scale: two robots' maps of the same place (800 segments with 768-d descriptors along 670 m of a loop; the second robot sees 90 %
of them, every centre a few cm off, the descriptor slightly off, ids of its own: `own_view`), 64 submap centres each (10 m apart,
radius 15 m, at most 40 segments per submap: the reference's demo scale, some 15-40 objects a submap), no submap descriptor and no
skip distance: every pair of the 64 x 64 grid is registered.  cosine_min 0.5, epsilon_shape 0.

The driver starts every GPU step as a child process under its own `timeout -k 10` and stops at the first non-zero status:
  pools    (a) submap_align_pools with the device-prefilter plugin (DistRegWithPruning.on_device()) over pools built with it;
  grid     (b) what a caller holding such pools had before: SubmapPool.to_submaps() + submap_align_grid with the factory's plugin
           (the NumPy prefilter per pair, every submap packed and uploaded again), on the same pools;
           both: the median of --reps calls after --warmup, results on the host; the pools are built once, outside the timing;
  caps     which problems of that batch k_small can finish: the same 4096 problems through roman_align_batch (host pointers, so
           that the per-problem statistics come back), n_live and nnz_upper of every problem as the DEVICE counted them, against
           k_small's caps (SMALL_MAXL live associations, COO_CAP stored pairs) — for the device-prefilter plugin and, over pools
           of the same submaps packed by method='roman', for a RomanRegistration: is a pruned problem left behind more often?
  trace    --warmup calls and ONE more of (a) under `rocprofv3 --kernel-trace --stats`, in a run of its own -> <out>/rocprof/;
           the driver then cuts the trace at the last launch of the gate kernel and writes the per-kernel table of that ONE call
           (<out>/kernels_one_call.csv): k_small, or the general chain?
-> <out>/timing.json.  No ratio is promised: the numbers are what they are."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 768
LIMITS = dict(pools=300, grid=840, caps=300, trace=300)    # seconds per step
SMALL_MAXL, COO_CAP = 128, 384                             # kernels.hip.h: what k_small takes (live associations, stored pairs)


def own_view(segs, r, keep=0.9):
    """Robot r's own map of the place: a random `keep` fraction of the segments, every centre a few cm off, the descriptor slightly
    off, ids of its own (what tests/_session.robot_view does for the session tests)."""
    import copy
    import numpy as np
    rng = np.random.default_rng(9000 + r)
    pick = np.sort(rng.permutation(len(segs))[:max(1, int(round(keep * len(segs))))])
    out = []
    for k in pick.tolist():
        q = copy.deepcopy(segs[k])
        q.id = int(segs[k].id) + 100000 * r
        q.centroid = np.asarray(q.centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(q.centroid))
        v = np.asarray(q.semantic_descriptor, dtype=np.float64) + 0.02 * rng.standard_normal(D) / np.sqrt(D)
        q.semantic_descriptor = v / np.linalg.norm(v)
        out.append(q)
    return out


def setup(method="clipper+prune"):
    """-> (torch, dev, ctx, params, io, host plugin, device plugin, pools, segment lists).  `method` 'roman': the same submaps packed
    by a RomanRegistration (both plugins are then that registration)."""
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method=method, semantics_dim=D, cosine_min=0.5, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    host = p.get_object_registration(); host.set_context(ctx)
    reg = host.on_device(D) if method == "clipper+prune" else host
    params = SubmapParams.from_submap_align_params(p)
    pools, segs = [], []
    for r in range(2):                                        # the same place mapped by two robots: cross pairs have true matches
        sg, traj, times = synth.make_map(800, D, seed=8100, n_poses=1280, loop_radius=80.0, laps=1.34, dt=1.0)
        if r == 1:
            sg = own_view(sg, r)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=ctx, device=dev))
        segs.append(sg)
    return torch, dev, ctx, p, io, host, reg, pools, segs


def digest(res):
    import numpy as np
    n = np.nan_to_num(res.clipper_num_associations, nan=-1.0)
    return dict(registered=len(res.timing_list), aligned=int((n >= 4).sum()), associations=int(n[n > 0].sum()), loop_closures=int(len(res.lc_edges["pairs"])))


def step_path(a, which):
    import numpy as np
    from roman_amd.align import submap_align as sa
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    sec = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if which == "pools":
            res = sa.submap_align_pools(p, pools, io, registration=reg)
            t1 = t0
        else:
            subs = [q.to_submaps(s) for q, s in zip(pools, segs)]
            t1 = time.perf_counter()
            res = sa.submap_align_grid(p, subs, io, registration=host)
        t2 = time.perf_counter()
        print(f"[{which}] call {rep}: {t2 - t0:.3f} s", file=sys.stderr, flush=True)
        if rep >= a.warmup:
            sec.append(dict(to_submaps=t1 - t0, align=t2 - t1, total=t2 - t0))
    out = {k + "_s": float(statistics.median(x[k] for x in sec)) for k in sec[0]}
    objs = np.concatenate([q.count[q.nonempty] for q in pools])
    out.update(total_s_all=[x["total"] for x in sec], submaps=[int(len(q.nonempty)) for q in pools], objects_per_submap=[int(objs.min()), float(objs.mean()), int(objs.max())],
               row_width=int(pools[0].pool.shape[1]), **digest(res))
    ctx.close()
    print("STEP_RESULT " + json.dumps(out), flush=True)


def step_caps(a):
    """n_live and nnz_upper of every problem of the grid as the device counted them, against k_small's caps."""
    import numpy as np
    from roman_amd.align import batch as rb
    out = {}
    for method in ("clipper+prune", "roman"):
        torch, dev, ctx, p, io, host, reg, pools, segs = setup(method)
        bt, pool = pools[0].grid_batch(pools[1])
        bt.feats = pool.cpu().numpy()
        res = rb.run_batch(reg, bt, ctx=ctx)
        L, nz = res.stats["n_live"].astype(np.int64), res.stats["nnz_upper"].astype(np.int64)
        n = np.array([len(x) for x in res.assoc])
        long_list, many_pairs = L > SMALL_MAXL, (L <= SMALL_MAXL) & (nz > COO_CAP)
        out[method] = dict(problems=int(len(L)), n_live_median=float(np.median(L)), n_live_max=int(L.max()), nnz_upper_median=float(np.median(nz)),
                           nnz_upper_max=int(nz.max()), aligned=int((n >= 4).sum()), over_small_maxl=int(long_list.sum()),
                           within_small_maxl_over_coo_cap=int(many_pairs.sum()), of_those_aligned=int((many_pairs & (n >= 4)).sum()),
                           within_both_caps=int((~long_list & ~many_pairs).sum()))
        ctx.close()
    out["caps"] = dict(SMALL_MAXL=SMALL_MAXL, COO_CAP=COO_CAP, note="k_small also leaves a problem with more than 2304 candidate pairs; a problem within COO_CAP "
                       "stored pairs has at most that many candidates above affinityeps, so that cap is not counted separately")
    print("STEP_RESULT " + json.dumps(out), flush=True)


def step_one(a):
    from roman_amd.align import submap_align as sa
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    for _ in range(a.warmup + 1):
        sa.submap_align_pools(p, pools, io, registration=reg)
    ctx.close()


def short_name(name):
    """A kernel's name without return type, namespace noise and argument list: cut at the first '(' outside template brackets."""
    n = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("roman::", "")
    depth = 0
    for i, ch in enumerate(n):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return n[:i]
    return n


def kernels_of_the_last_call(trace_csv):
    """The launches behind the LAST launch of the gate kernel -> [(kernel, launches, total us)], in order of first launch."""
    rows = list(csv.DictReader(open(trace_csv)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short_name(r["Kernel_Name"])) for r in rows)
    gates = [i for i, e in enumerate(ev) if e[2].startswith("k_grid_gate")]
    table = {}
    for s, e, n in ev[gates[-1]:] if gates else []:
        c = table.setdefault(n, [0, 0.0]); c[0] += 1; c[1] += (e - s) / 1e3
    return [(n, c[0], c[1]) for n, c in table.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["pools", "grid", "caps", "one"], default=None, help="(internal) run one step in this process")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_pools"))
    a = ap.parse_args()
    if a.step in ("pools", "grid"):
        return step_path(a, a.step)
    if a.step == "caps":
        return step_caps(a)
    if a.step == "one":
        return step_one(a)
    out_dir = os.path.abspath(a.out)
    os.makedirs(out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    rec = dict(scale=dict(d=D, cosine_min=0.5, submap_max_size=40, reps=a.reps, warmup=a.warmup))
    for step, key in (("pools", "pools_device_prefilter"), ("grid", "to_submaps_grid_host_prefilter"), ("caps", "k_small_caps")):
        print(f"[gpu_prune_pools] step {step}", flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step])] + me + ["--step", step], cwd=ROOT, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
            print(f"[gpu_prune_pools] step {step} ended with status {r.returncode}: stopping\n{r.stdout[-2000:]}", flush=True)
            return r.returncode or 1
        rec[key] = json.loads(line[0][len("STEP_RESULT "):])
        print(step, line[0], flush=True)
    a_, b_ = rec["pools_device_prefilter"], rec["to_submaps_grid_host_prefilter"]
    rec["same_counts"] = all(a_[k] == b_[k] for k in ("registered", "aligned", "associations", "loop_closures"))
    with open(os.path.join(out_dir, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print("[gpu_prune_pools] step trace", flush=True)
    prof = os.path.join(out_dir, "rocprof")
    rc = subprocess.call(["timeout", "-k", "10", str(LIMITS["trace"]), "rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "prune_pools", "--output-format", "csv", "--"]
                         + me + ["--step", "one"], cwd=ROOT)
    if rc != 0:
        print(f"[gpu_prune_pools] step trace ended with status {rc}: stopping", flush=True)
        return rc
    traces = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    if traces:
        table = kernels_of_the_last_call(traces[0])
        with open(os.path.join(out_dir, "kernels_one_call.csv"), "w") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "launches", "total_us"])
            for n, c, us in table:
                w.writerow([n, c, f"{us:.1f}"])
        rec["one_call_kernels"] = [dict(kernel=n, launches=c, total_us=round(us, 1)) for n, c, us in table]
        with open(os.path.join(out_dir, "timing.json"), "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec), flush=True)
    return 0 if rec["same_counts"] else 2


if __name__ == "__main__":
    sys.exit(main() or 0)
