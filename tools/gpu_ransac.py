#!/usr/bin/env python3
"""Batched RANSAC registration (roman_ransac_batch_dev, method 'ransac') on 4096 distinct demo-scale pairs (n = m = 20 ... 40
objects, the submap grid of tools/gpu_demo_scale.py without descriptors) at ransac_iter 10^4 and 10^6.  Not a test and not bench.py.

    python tools/gpu_ransac.py [--pairs 4096] [--commit HASH]

The driver starts every GPU step as a child process under its own `timeout -k 10` and stops at the first non-zero status:
  time     per ransac_iter: warm-up calls, then the median of repeated device-pointer calls timed with events on the context's
           stream (the call is a pure enqueue); pairs/s, and from the records the hypotheses generated (n_hyp) and scored (n_scored).
           The only comparison is the NumPy oracle (tests/_ransac_oracle.py) on a few of the same pairs on the same machine, per
           hypothesis.  -> profiles/ransac/timing.json
  trace    one call at ransac_iter 10^4 under `rocprofv3 --kernel-trace --stats`, in a process of its own -> profiles/ransac/rocprof/
The kernel's register / LDS / scratch figures come from tools/kernel_resources.py (no GPU needed).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ransac")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def grid(n_pairs):
    """-> (reg, AlignmentBatch over a pool of object centres): 64 x 64 submaps of 20 ... 40 objects, half of them shared landmarks."""
    import numpy as np
    from roman_amd import synth
    from roman_amd.align import RansacReg
    from roman_amd.align import batch as rb
    reg = RansacReg()
    rng = np.random.default_rng(5000)
    SD = 64
    subs, _ = synth.make_submap_grid(2 * SD, n=40, d=0, seed0=5000)
    sizes = rng.integers(20, 41, size=2 * SD)
    subs = [sm[:int(k)] for sm, k in zip(subs, sizes)]
    bt = rb.batch_from_submap_grid(reg, subs[:SD], subs[SD:])
    if n_pairs < len(bt):
        bt = bt.subset(0, n_pairs)
    return reg, bt


def step_time(args):
    import numpy as np
    import torch
    from roman_amd import _abi
    from roman_amd.runtime import Context, ransac_record_dtype
    reg, bt = grid(args.pairs)
    B = len(bt)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    kmax = 64
    pts = torch.from_numpy(bt.feats).cuda()
    a_out = torch.zeros((B, kmax, 2), dtype=torch.int32, device="cuda")
    rec_out = torch.zeros(B * _abi.RANSAC_RECORD_NBYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rec = dict(commit=args.commit, pairs=B, objects_per_map="20-40", mean_correspondences=float(np.mean(bt.n1.astype(np.int64) * bt.n2)),
               round=reg.round, edge_len=reg.edge_len, max_dist=reg.max_dist, confidence=reg.confidence, kmax=kmax)
    for iters, warm, reps in ((10 ** 4, 2, 10), (10 ** 6, 1, 5)):
        reg.max_iteration = iters
        P = reg._ransac_params()

        def call():
            ctx.ransac_batch_dev(P, pts.data_ptr(), bt.off1, bt.n1, bt.off2, bt.n2, kmax, a_out.data_ptr(), rec_out.data_ptr())
        with torch.cuda.stream(stream):
            for _ in range(warm):
                call()
            stream.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); call(); e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        r = np.frombuffer(rec_out.cpu().numpy().tobytes(), dtype=ransac_record_dtype())
        med = statistics.median(ms)
        n_hyp, n_scored = int(r["n_hyp"].sum()), int(r["n_scored"].sum())
        rec[f"ransac_iter_{iters}"] = dict(
            ms_per_call=med, ms_all=ms, timed_calls=reps, warmup_calls=warm, pairs_per_s=B / (med * 1e-3),
            hypotheses_generated=n_hyp, hypotheses_scored=n_scored, scored_share=n_scored / max(n_hyp, 1),
            hypotheses_generated_per_s=n_hyp / (med * 1e-3), hypotheses_scored_per_s=n_scored / (med * 1e-3),
            pairs_stopped_early=int((r["n_hyp"] < iters).sum()), mean_n_hyp=float(r["n_hyp"].mean()), max_n_hyp=int(r["n_hyp"].max()),
            mean_best_count=float(r["best_count"].mean()), pairs_with_pose=int((r["status"] == 0).sum()))
        print(f"ransac_iter {iters}: {med:.3f} ms per call of {B} pairs, {B / (med * 1e-3):.0f} pairs/s, generated {n_hyp}, scored {n_scored} "
              f"({100.0 * n_scored / max(n_hyp, 1):.3f} %), stopped early {rec[f'ransac_iter_{iters}']['pairs_stopped_early']}", flush=True)
    # the NumPy oracle on a few of the same pairs, same machine: seconds per generated hypothesis
    import _ransac_oracle as ro
    idx = np.linspace(0, B - 1, args.oracle_pairs).astype(int)
    t0 = time.perf_counter(); nh = 0
    for b in idx:
        Pm = bt.feats[bt.off1[b]:bt.off1[b] + bt.n1[b]]; Qm = bt.feats[bt.off2[b]:bt.off2[b] + bt.n2[b]]
        nh += ro.run(Pm, Qm, max_iteration=10 ** 4, round=reg.round, edge_len=reg.edge_len, max_dist=reg.max_dist, confidence=reg.confidence, seed=reg.seed).n_hyp
    dt = time.perf_counter() - t0
    dev = rec["ransac_iter_10000"]
    rec["numpy_oracle"] = dict(pairs_timed=len(idx), ransac_iter=10 ** 4, hypotheses=nh, seconds=dt, us_per_hypothesis=dt / max(nh, 1) * 1e6,
                               device_us_per_hypothesis=dev["ms_per_call"] * 1e3 / max(dev["hypotheses_generated"], 1),
                               note="one CPU core, pure NumPy / Python integers; per generated hypothesis, not the whole batch")
    print(f"NumPy oracle: {rec['numpy_oracle']['us_per_hypothesis']:.2f} us per hypothesis on {len(idx)} pairs; device {rec['numpy_oracle']['device_us_per_hypothesis']:.5f} us", flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


def step_one(args):
    from roman_amd.align import batch as rb
    from roman_amd.runtime import Context
    reg, bt = grid(args.pairs)
    reg.max_iteration = 10 ** 4
    ctx = Context(0); reg.set_context(ctx)
    for _ in range(2):
        rb.run_batch(reg, bt)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--oracle-pairs", type=int, default=4)
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
    me = [sys.executable, os.path.abspath(__file__), "--pairs", str(args.pairs), "--oracle-pairs", str(args.oracle_pairs), "--commit", args.commit]
    steps = [
        ("time", ["timeout", "-k", "10", "420"] + me + ["--step", "time"]),
        ("trace", ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(OUT, "rocprof"), "-o", "ransac", "--output-format", "csv", "--"] + me + ["--step", "one"]),
    ]
    for name, cmd in steps:
        print(f"[gpu_ransac] step {name}", flush=True)
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print(f"[gpu_ransac] step {name} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
