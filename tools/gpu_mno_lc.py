#!/usr/bin/env python3
"""Multi-hypothesis loop closures over device-resident pools.  Not a test and not bench.py.

    python tools/gpu_mno_lc.py [--out profiles/mno_lc] [--reps 10] [--warmup 3]

Scale: the 64 x 64 grid of tools/gpu_prune_pools.py at the reference's demo scale — two robots' maps of the same place (800
segments with 768-d descriptors, the second robot's own view of 90 % of them), 64 submaps each of some 15-40 objects, method
'roman', no submap descriptor, no skip distance: all 4096 pairs are registered.

The driver starts every GPU step as a child process under its own `timeout -k 10` and stops at the first non-zero status:
  pools K  submap_align_pools over the resident pools with num_solutions = K (none: the single-solution path), K = none, 1, 2, 3;
  tail     roman_mno_lc_tail_dev alone over the 4096 x 3 solutions of one roman_mno_batch_dev pass, between two events on the
           context's stream;
  old      the only way to the same results before: SubmapPool.to_submaps(), mno_clipper_batch over all pairs (K = 2), and the
           tail per hypothesis in NumPy (the vectorised statement of tests/_lc_tail.py over the flattened poses — kinder to the
           old way than a Python loop per pair — plus the best rule);
           all: the median of --reps calls after --warmup, results on the host; the pools are built once, outside the timing;
  trace    --warmup calls and one more of `pools 2` under `rocprofv3 --kernel-trace --stats`, no counters, in a run of its own
           -> <out>/rocprof/; its per-kernel table is kept as <out>/kernel_stats.csv.
-> <out>/timing.json.  No ratio is promised: the numbers are what they are."""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = dict(pools=300, tail=300, old=600, trace=300)       # seconds per step
K_OLD, K_TAIL = 2, 3


def setup():
    import gpu_prune_pools as pp
    return pp.setup("roman")


def digest(res):
    import numpy as np
    n = np.nan_to_num(res.clipper_num_associations, nan=-1.0)
    return dict(registered=len(res.timing_list), aligned=int((n >= 4).sum()), associations=int(n[n > 0].sum()), loop_closures=int(len(res.lc_edges["pairs"])))


def med(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def step_pools(a):
    from roman_amd.align import submap_align as sa
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    K = None if a.k == 0 else a.k
    sec = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=K)
        t1 = time.perf_counter()
        print(f"[pools K={K}] call {rep}: {t1 - t0:.3f} s", file=sys.stderr, flush=True)
        if rep >= a.warmup:
            sec.append(t1 - t0)
    out = dict(med(sec), **digest(res))
    if K is not None:
        flags = [h[4] for hyps in res.hypotheses.values() for h in hyps]
        out["accepted_hypotheses"] = int(sum(1 for f in flags if f & 1))
    ctx.close()
    print("STEP_RESULT " + json.dumps(out), flush=True)


def step_tail(a):
    """The tail alone: one pass of the K solves leaves the solutions in HBM; then the tail between two events, per call."""
    import numpy as np
    from roman_amd import _abi
    from roman_amd.align import submap_align as sa
    from roman_amd.align.pipeline import issue_mno_chunked
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    K = K_TAIL
    batch, pool = pools[0].grid_batch(pools[1])
    B, kmax = len(batch), batch.kmax()
    i32 = torch.int32
    a_out = torch.full((B, K, kmax, 2), -1, dtype=i32, device=dev)
    sol = torch.zeros(B * K * _abi.MNO_SOLUTION_NBYTES, dtype=torch.uint8, device=dev)
    rec = torch.zeros(B * K * _abi.LC_RECORD_NBYTES, dtype=torch.uint8, device=dev)
    best = torch.zeros(B, dtype=i32, device=dev); idx = torch.zeros(B * K, dtype=i32, device=dev); cnt = torch.zeros(1, dtype=i32, device=dev)
    bidx = torch.zeros(B, dtype=i32, device=dev); bcnt = torch.zeros(1, dtype=i32, device=dev)
    eye = np.tile(np.eye(4).reshape(1, 16), (B, 1))
    T_ref = torch.from_numpy(eye).to(dev); enable = torch.ones(B, dtype=i32, device=dev)
    S = max(len(q.nonempty) for q in pools)
    frames = torch.from_numpy(np.tile(np.eye(4).reshape(1, 16), (S, 1))).to(dev)
    pi = torch.from_numpy(np.ascontiguousarray(batch.pair_index.astype(np.int32))).to(dev)
    iL, iR = pi[:, 0].contiguous(), pi[:, 1].contiguous()
    torch.cuda.synchronize(dev)
    status = issue_mno_chunked(ctx, reg._abi_params(), pool, batch, K, kmax, a_out, sol)
    ctx.join(); ctx.sync()
    lp = sa._lc_inputs(p, io, reg).params()
    stream = torch.cuda.current_stream(dev)
    ms = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.mno_lc_tail_dev(lp, B, K, sol.data_ptr(), rec.data_ptr(), best.data_ptr(), idx.data_ptr(), cnt.data_ptr(), bidx.data_ptr(), bcnt.data_ptr(),
                            T_ref_ptr=T_ref.data_ptr(), enable_ptr=enable.data_ptr(), FL_ptr=frames.data_ptr(), iL_ptr=iL.data_ptr(),
                            FR_ptr=frames.data_ptr(), iR_ptr=iR.data_ptr())
        e1.record(stream)
        ctx.sync(); torch.cuda.synchronize(dev)
        if rep >= a.warmup:
            ms.append(e0.elapsed_time(e1) / 1e3)
    out = dict(med(ms), problems=B, K=K, skipped=int((status & _abi.ROMAN_ST_WORKSPACE != 0).sum()), accepted=int(cnt.cpu().numpy()[0]),
               accepted_best=int(bcnt.cpu().numpy()[0]), launches="k_mno_lc_tail, k_lc_compact, k_mno_best_compact")
    ctx.close()
    print("STEP_RESULT " + json.dumps(out), flush=True)


def step_old(a):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _mno_lc as ml
    from roman_amd.align import submap_align as sa
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    K = K_OLD
    sec = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        subs = [q.to_submaps(s) for q, s in zip(pools, segs)]
        t1 = time.perf_counter()
        n0, n1 = len(subs[0]), len(subs[1])
        pairs = [(subs[0][i].segments, subs[1][j].segments) for i in range(n0) for j in range(n1)]
        sols, poses, res = reg.mno_clipper_batch(pairs, num_solutions=K, return_result=True)
        t2 = time.perf_counter()
        Tw = [np.stack([np.array(sm.pose_gravity_aligned) for sm in subs[r]]) for r in range(2)]
        fr = [[sa._edge_frames(sm) for sm in subs[r]] for r in range(2)]
        iL, iR = np.divmod(np.arange(n0 * n1), n1)
        lc = sa._lc_inputs(p, io, reg, T_ref=np.matmul(np.linalg.inv(Tw[0])[:, None], Tw[1][None]).reshape(-1, 4, 4), enable=np.ones(n0 * n1, np.int32),
                           FL=np.stack([f[0] for f in fr[0]]), iL=iL, FR=np.stack([f[1] for f in fr[1]]), iR=iR)
        n_assoc = np.array([[len(s[0]) for s in one] for one in sols], dtype=np.int32)
        rec, best, acc, acc_best = ml.mno_lc_tail(lc, K, res.T, n_assoc, res.status)
        t3 = time.perf_counter()
        print(f"[old] call {rep}: {t3 - t0:.3f} s", file=sys.stderr, flush=True)
        if rep >= a.warmup:
            sec.append(dict(to_submaps=t1 - t0, mno_clipper_batch=t2 - t1, numpy_tail=t3 - t2, total=t3 - t0))
    n_best = rec["n_assoc"].reshape(-1, K)[np.arange(len(best)), np.maximum(best, 0)]
    out = dict(med([x["total"] for x in sec]), K=K, **{k + "_median_s": float(statistics.median(x[k] for x in sec)) for k in ("to_submaps", "mno_clipper_batch", "numpy_tail")},
               registered=int(len(best)), aligned=int((n_best >= 4).sum()), associations=int(n_best.sum()), loop_closures=int(len(acc_best)),
               accepted_hypotheses=int(len(acc)))
    ctx.close()
    print("STEP_RESULT " + json.dumps(out), flush=True)


def step_one(a):
    from roman_amd.align import submap_align as sa
    torch, dev, ctx, p, io, host, reg, pools, segs = setup()
    for _ in range(a.warmup + 1):
        sa.submap_align_pools(p, pools, io, registration=reg, num_solutions=2)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["pools", "tail", "old", "one"], default=None, help="(internal) run one step in this process")
    ap.add_argument("--k", type=int, default=0, help="(internal) num_solutions of the pools step; 0: none")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mno_lc"))
    a = ap.parse_args()
    if a.step:
        return dict(pools=step_pools, tail=step_tail, old=step_old, one=step_one)[a.step](a)
    out_dir = os.path.abspath(a.out)
    os.makedirs(out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    rec = dict(scale=dict(grid="64 x 64", method="roman", d=768, submap_max_size=40, reps=a.reps, warmup=a.warmup))
    steps = [("pools", ["--k", str(k)], f"pools_num_solutions_{k if k else 'none'}") for k in (0, 1, 2, 3)]
    steps += [("tail", [], "tail_alone"), ("old", [], "old_way_to_submaps_mno_clipper_batch_numpy_tail")]
    for step, extra, key in steps:
        print(f"[gpu_mno_lc] step {key}", flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step])] + me + ["--step", step] + extra, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
            print(f"[gpu_mno_lc] step {key} ended with status {r.returncode}: stopping\n{r.stdout[-2000:]}", flush=True)
            return r.returncode or 1
        rec[key] = json.loads(line[0][len("STEP_RESULT "):])
        print(key, line[0][:400], flush=True)
        with open(os.path.join(out_dir, "timing.json"), "w") as f:
            json.dump(rec, f, indent=1)
    new, old = rec[f"pools_num_solutions_{K_OLD}"], rec["old_way_to_submaps_mno_clipper_batch_numpy_tail"]
    rec["old_over_new_at_K"] = dict(K=K_OLD, ratio=old["median_s"] / new["median_s"])
    rec["same_counts"] = all(new[k] == old[k] for k in ("registered", "aligned", "associations", "loop_closures", "accepted_hypotheses"))
    with open(os.path.join(out_dir, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print("[gpu_mno_lc] step trace", flush=True)
    prof = os.path.join(out_dir, "rocprof")
    rc = subprocess.call(["timeout", "-k", "10", str(LIMITS["trace"]), "rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "mno_lc", "--output-format", "csv", "--"]
                         + me + ["--step", "one"], cwd=ROOT)
    if rc != 0:
        print(f"[gpu_mno_lc] step trace ended with status {rc}: stopping", flush=True)
        return rc
    stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    if stats:
        shutil.copyfile(stats[0], os.path.join(out_dir, "kernel_stats.csv"))
    print(json.dumps({k: v for k, v in rec.items() if k != "scale"})[:3000], flush=True)
    return 0 if rec["same_counts"] else 2


if __name__ == "__main__":
    sys.exit(main() or 0)
