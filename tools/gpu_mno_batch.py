#!/usr/bin/env python3
"""Batched multi-solution extraction (roman_mno_batch) against the per-pair mno_clipper() loop, on the 4096 distinct demo-scale
pairs of tools/gpu_demo_scale.py's grid (method 'roman', 20-40 objects per map, d = 768).  Not a test and not bench.py.

    python tools/gpu_mno_batch.py [--pairs 4096] [--loop-pairs 16] [--commit HASH]

The driver starts every GPU step as a child process under its own `timeout -k 10` and stops at the first non-zero status:
  time     median of >= 10 timed calls after warm-up, result on the host: run_mno_batch with num_solutions 1, 2, 3, run_batch on the
           same batch, and the per-pair mno_clipper(num_solutions=2) loop on a subset of the same pairs -> profiles/mno_batch/timing.json
  trace    one batched call (num_solutions = 2) under `rocprofv3 --kernel-trace --stats`, in a process of its own -> profiles/mno_batch/rocprof/
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "mno_batch")
sys.path.insert(0, ROOT)


def grid(n_pairs):
    import numpy as np
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import batch as rb
    from roman_amd.runtime import Context
    ctx = Context(0)
    reg = SubmapAlignParams(method="roman", semantics_dim=768).get_object_registration(); reg.set_context(ctx)
    rng = np.random.default_rng(5000)
    SD = 64
    subs, _ = synth.make_submap_grid(2 * SD, n=40, d=768, seed0=5000)
    sizes = rng.integers(20, 41, size=2 * SD)
    subs = [sm[:int(k)] for sm, k in zip(subs, sizes)]
    bt = rb.batch_from_submap_grid(reg, subs[:SD], subs[SD:])
    if n_pairs < len(bt):
        bt = bt.subset(0, n_pairs)
    return ctx, reg, rb, bt, subs, SD


def timed(fn, n=10, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def step_time(args):
    import numpy as np
    ctx, reg, rb, bt, subs, SD = grid(args.pairs)
    B = len(bt)
    rec = dict(commit=args.commit, pairs=B, method="roman", d=768, objects_per_map="20-40", timed_calls=10)
    for K in (1, 2, 3):
        res = [None]
        med, ts = timed(lambda: res.__setitem__(0, rb.run_mno_batch(reg, bt, K)))
        st = res[0].stats
        rec[f"mno_batch_K{K}"] = dict(ms_per_call=med * 1e3, us_per_pair=med / B * 1e6, ms_all=[t * 1e3 for t in ts],
                                      mean_passes_per_round=[float(st["n_pass"][:, k].mean()) for k in range(K)],
                                      max_passes_per_round=[int(st["n_pass"][:, k].max()) for k in range(K)],
                                      mean_associations_per_round=[float(np.mean([len(a[k]) for a in res[0].assoc])) for k in range(K)],
                                      mean_nodes=float(st["n_live"][:, 0].mean()), mean_nnz_upper=float(st["nnz_upper"][:, 0].mean()))
        print(f"run_mno_batch K={K}: {med * 1e3:.3f} ms per call, {med / B * 1e6:.2f} us per pair, passes per round {rec[f'mno_batch_K{K}']['mean_passes_per_round']}", flush=True)
    med, ts = timed(lambda: rb.run_batch(reg, bt))
    rec["run_batch"] = dict(ms_per_call=med * 1e3, us_per_pair=med / B * 1e6, ms_all=[t * 1e3 for t in ts])
    print(f"run_batch: {med * 1e3:.3f} ms per call", flush=True)
    idx = np.linspace(0, B - 1, args.loop_pairs).astype(int)
    pairs = [(subs[bt.pair_index[b][0]], subs[SD + bt.pair_index[b][1]]) for b in idx]
    reg.mno_clipper(*pairs[0], num_solutions=2)                # warm-up
    per = []
    for m1, m2 in pairs:
        t0 = time.perf_counter(); reg.mno_clipper(m1, m2, num_solutions=2); per.append(time.perf_counter() - t0)
    loop = statistics.median(per)
    rec["mno_clipper_loop_K2"] = dict(pairs_timed=len(pairs), ms_per_pair_median=loop * 1e3, ms_per_pair_mean=statistics.mean(per) * 1e3, ms_all=[t * 1e3 for t in per])
    rec["ratio_loop_over_batch_K2_per_pair"] = loop / (rec["mno_batch_K2"]["ms_per_call"] / 1e3 / B)
    print(f"mno_clipper loop: {loop * 1e3:.2f} ms per pair; batched K=2 {rec['mno_batch_K2']['us_per_pair']:.2f} us per pair; ratio {rec['ratio_loop_over_batch_K2_per_pair']:.0f}x", flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


def step_one(args):
    ctx, reg, rb, bt, subs, SD = grid(args.pairs)
    for _ in range(2):
        rb.run_mno_batch(reg, bt, 2)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--loop-pairs", type=int, default=16)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step", choices=["time", "one"], default=None)
    args = ap.parse_args()
    if args.commit is None:
        try:
            args.commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            args.commit = "unknown"
    if args.step == "time":
        return step_time(args)
    if args.step == "one":
        return step_one(args)
    os.makedirs(OUT, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--pairs", str(args.pairs), "--loop-pairs", str(args.loop_pairs), "--commit", args.commit]
    steps = [
        ("time", ["timeout", "-k", "10", "420"] + me + ["--step", "time"]),
        ("trace", ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(OUT, "rocprof"), "-o", "mno_batch", "--output-format", "csv", "--"] + me + ["--step", "one"]),
    ]
    for name, cmd in steps:
        print(f"[gpu_mno_batch] step {name}", flush=True)
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print(f"[gpu_mno_batch] step {name} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
