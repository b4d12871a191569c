#!/usr/bin/env python3
"""Times the segment-shape step on one MI355X and writes profiles/segment_shapes/timing.json, every
sample kept.  10 000 segments (the session of §6.19), three point-count distributions:
  loguniform   counts log-uniform in 16 ... 4096 — an ASSUMPTION: nobody here has measured the distribution of a real map
  all-64       every segment 64 points: the wave path alone
  all-4096     every segment 4096 points: the workgroup path alone
Per distribution: the device call alone between two events on the context's stream (roman_segment_shapes_dev on resident clouds
that every repetition reads again: WARM caches where the clouds fit them), for both centre references; MapTable.from_point_clouds end to end (upload, call, read-back); and the NumPy per-segment loop of the test oracle on
this machine's CPU (on a subsample, scaled: the loop is linear in the segments).  Reports the bytes of points per sweep over the
device time against the 8 TB/s HBM figure the other sections use, and the sweeps a call makes: 3 for 'mean' (mean, covariance,
box), 3 + 8 for 'bottom_middle' (eight radix-select passes).  A threshold sweep (roman_ctx_set_segment_block_min) over uniform
counts records where a workgroup starts to beat a wave."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8.0e12
N_SEG, WARMUP, REPS = 10000, 3, 20


def clouds_of(counts, rng):
    from roman_amd.align import SegmentClouds
    off = np.zeros(len(counts) + 1, dtype=np.int64); off[1:] = np.cumsum(counts)
    centres = rng.uniform(-200.0, 200.0, (len(counts), 3))
    pts = rng.uniform(-0.5, 0.5, (int(off[-1]), 3)) * (0.3, 1.1, 2.7) + np.repeat(centres, counts, axis=0)
    return SegmentClouds(pts, off, np.arange(len(counts), dtype=np.int64), np.zeros((len(counts), 2)), None)


def device_ms(torch, ctx, clouds, center_ref, reps=REPS):
    from roman_amd.runtime import segment_shape_params
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(clouds.points).to(dev); off = torch.from_numpy(clouds.seg_off).to(dev)
    out = torch.zeros((len(clouds), 10), dtype=torch.float64, device=dev); st = torch.zeros(len(clouds), dtype=torch.int32, device=dev)
    P = segment_shape_params(center_ref, 10, 0, 3, 6, 7)
    torch.cuda.synchronize()
    samples = []
    for k in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.sync()
        a.record()                                               # both events on the context's stream (torch's current one): the device alone,
        ctx.segment_shapes_dev(pts.data_ptr(), off.data_ptr(), clouds.seg_off, P, out.data_ptr(), st.data_ptr())
        b.record(); b.synchronize()                              # no host round trip inside the interval
        if k >= WARMUP:
            samples.append(a.elapsed_time(b))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_shapes", "timing.json"))
    args = ap.parse_args()
    import torch
    import _segment_shapes_oracle as so
    from roman_amd.align import RansacReg, SubmapAlignParams
    from roman_amd.align.submaps import MapTable
    from roman_amd.runtime import Context
    stream = torch.cuda.Stream(torch.device("cuda:0")); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(6240)
    result = {"n_segments": N_SEG, "hbm_bytes_per_s": HBM_BYTES_PER_S, "sweeps": {"mean": 3, "bottom_middle": 11},
              "assumption": "point counts log-uniform in 16 ... 4096: the distribution of a real map has not been measured", "cases": {}}
    dists = {"loguniform": np.exp(rng.uniform(np.log(16), np.log(4096), N_SEG)).astype(np.int64),
             "all-64": np.full(N_SEG, 64, dtype=np.int64), "all-4096": np.full(N_SEG, 4096, dtype=np.int64)}
    reg = SubmapAlignParams(method="pcavolgrav").get_object_registration(); reg.set_context(ctx)
    with torch.cuda.stream(stream):
        for name, counts in dists.items():
            clouds = clouds_of(counts, rng)
            case = {"points": int(clouds.seg_off[-1]), "bytes_per_sweep": int(clouds.seg_off[-1]) * 24}
            for ref in ("mean", "bottom_middle"):
                ms = device_ms(torch, ctx, clouds, ref)
                med = float(np.median(ms))
                case[f"device_ms_{ref}"] = ms
                case[f"device_ms_{ref}_median"] = med
                case[f"sweep_bytes_per_s_{ref}"] = case["bytes_per_sweep"] * result["sweeps"][ref] / (med * 1e-3)
            e2e = []
            for k in range(1 + 5):
                t0 = time.perf_counter(); MapTable.from_point_clouds(reg, clouds, ctx=ctx); e2e.append((time.perf_counter() - t0) * 1e3)
            case["from_point_clouds_ms"] = e2e[1:]
            sub = min(N_SEG, 500)
            t0 = time.perf_counter()
            for i in range(sub):
                so.segment(clouds.points[clouds.seg_off[i]:clouds.seg_off[i + 1]])
            case["numpy_loop_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * N_SEG / sub
            case["numpy_loop_subsample"] = sub
            result["cases"][name] = case
            print(name, {k: v for k, v in case.items() if not isinstance(v, list)}, flush=True)
        # where a workgroup starts to beat a wave: 2000 segments of n points each, every segment forced down either path
        sweep = {}
        for n in (128, 256, 384, 512, 768, 1024, 2048):
            clouds = clouds_of(np.full(2000, n, dtype=np.int64), rng)
            row = {}
            for path, t in (("wave", 1 << 30), ("block", 1)):
                ctx.set_segment_block_min(t)
                row[path] = device_ms(torch, ctx, clouds, "mean", reps=10)
            ctx.set_segment_block_min(0)
            sweep[str(n)] = row
            print("threshold", n, {p: float(np.median(v)) for p, v in row.items()}, flush=True)
        result["threshold_sweep_2000_segments"] = sweep
    out = args.out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)
    ctx.close()


if __name__ == "__main__":
    main()
