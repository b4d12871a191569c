#!/usr/bin/env python3
"""Submaps from a whole map on the device (roman_submaps_dev) on one map of about 10^4 segments with 768-d
descriptors and about 10^2 submap centres (radius 15 m, centres 10 m apart, max_size 40).  Not a test and not bench.py.

    python tools/gpu_submaps.py [--segments 10000] [--out profiles/submaps] [--commit HASH]

The driver starts the GPU step as a child process under its own `timeout -k 10` and reports its status.  The step times
  device   warm-up calls, then the median of repeated device-pointer calls timed with events on the context's stream (the call
           is a pure enqueue; the map table is already resident), and the upload of the table once, by a host clock around
           the copy and a synchronise;
  numpy    the NumPy restatement of the contract (tests/_submaps_oracle.py) on the same map, same machine, one core;
  host     the existing host path to the same pool: SubmapPool.to_submaps (segment views) -> pack_submaps.
The comparison is against the host paths on the same box, not against an earlier version of the device code.
-> <out>/timing.json.  Register / LDS / scratch figures: tools/kernel_resources.py (no GPU needed).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def step_time(args):
    import numpy as np
    import torch
    import _submaps_oracle as so
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align.batch import pack_submaps
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_call_params, submap_centers
    from roman_amd.runtime import Context
    d = 768
    segs, traj, times = synth.make_map(args.segments, d, seed=8200, n_poses=1000, loop_radius=125.0, laps=1.3, dt=1.0)
    reg = SubmapAlignParams(method="roman", semantics_dim=d).get_object_registration()
    params = SubmapParams(max_size=40, radius=15.0, distance=10.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor='mean_semantic')
    t0 = time.perf_counter(); table = MapTable.from_segments(reg, segs); t_table = time.perf_counter() - t0
    centers = submap_centers(traj, times, params)
    S, N, F = len(centers), len(table), table.feats.shape[1]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream); reg.set_context(ctx)
    P = submap_call_params(table, params)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    feats = torch.from_numpy(table.feats).to(dev); tms = torch.from_numpy(table.times).to(dev); ids = torch.from_numpy(table.ids).to(dev)
    torch.cuda.synchronize(dev); t_upload = time.perf_counter() - t0
    rows, Fo = S * P.cap, P.point_dim + F - 3
    pool = torch.zeros((rows, Fo), dtype=torch.float64, device=dev)
    count = torch.zeros(S, dtype=torch.int32, device=dev); status = torch.zeros(S, dtype=torch.int32, device=dev)
    src = torch.zeros(rows, dtype=torch.int32, device=dev); ids_out = torch.zeros(rows, dtype=torch.int64, device=dev)
    desc = torch.zeros((S, d), dtype=torch.float64, device=dev)
    descs = centers.descs()
    torch.cuda.synchronize(dev)

    def call():
        ctx.submaps_dev(P, N, F, feats.data_ptr(), tms.data_ptr(), descs, pool.data_ptr(), count.data_ptr(), src.data_ptr(), status.data_ptr(),
                        seg_ids_ptr=ids.data_ptr(), ids_out_ptr=ids_out.data_ptr(), desc_dim=d, desc_out_ptr=desc.data_ptr())
    ms = []
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            call()
        stream.synchronize()
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    cnt = count.cpu().numpy()
    # the NumPy restatement on the same map
    t0 = time.perf_counter()
    o = so.submaps_oracle(table.feats, table.times, descs, point_dim=3, max_size=40, prune_by_time=False, radius=15.0, seg_ids=table.ids, desc_dim=d)
    t_numpy = time.perf_counter() - t0
    src_h = src.cpu().numpy().reshape(S, P.cap)
    same = bool(np.array_equal(o["count"], cnt) and all(np.array_equal(o["src"][s, :cnt[s]], src_h[s, :cnt[s]]) for s in range(S)))
    # the existing host path to the same pool: segment views -> pack_submaps
    sp = build_submap_pool(reg, table, centers, params, ctx=ctx, device=dev)
    t0 = time.perf_counter(); sms = sp.to_submaps(segs); t_views = time.perf_counter() - t0
    t0 = time.perf_counter(); hf, ho = pack_submaps(reg, [sm.segments for sm in sms]); t_pack = time.perf_counter() - t0
    moved = int(cnt.sum()) * (F + Fo) * 8
    rec = dict(commit=args.commit, segments=N, centres=S, F=F, descriptor_dim=d, max_size=40, radius=15.0, rows_selected=int(cnt.sum()),
               mean_rows_per_submap=float(cnt.mean()), device=dict(ms_per_call=med, ms_all=ms, timed_calls=args.reps, warmup_calls=args.warmup,
                                                                   gathered_bytes_read_plus_written=moved, gather_gb_per_s_of_call_time=moved / (med * 1e-3) / 1e9,
                                                                   note="events on the context's stream around one pure-enqueue call: descriptor upload + 4 kernels; table resident"),
               table_upload_s=t_upload, table_bytes=int(table.feats.nbytes + table.times.nbytes + table.ids.nbytes),
               host=dict(map_table_from_segments_s=t_table, numpy_restatement_s=t_numpy, numpy_equals_device_selection=same,
                         to_submaps_s=t_views, pack_submaps_s=t_pack, to_submaps_plus_pack_s=t_views + t_pack, packed_rows=int(hf.shape[0]),
                         note="one CPU core of the same machine, Python / NumPy"))
    print(json.dumps(rec, indent=1), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "submaps"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step", choices=["time"], default=None)
    args = ap.parse_args()
    if args.commit is None:
        try:
            args.commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            args.commit = "unknown"
    if args.step == "time":
        return step_time(args)
    me = [sys.executable, os.path.abspath(__file__), "--segments", str(args.segments), "--warmup", str(args.warmup), "--reps", str(args.reps),
          "--out", args.out, "--commit", args.commit]
    print("[gpu_submaps] step time", flush=True)
    rc = subprocess.call(["timeout", "-k", "10", "420"] + me + ["--step", "time"], cwd=ROOT)
    if rc != 0:
        print(f"[gpu_submaps] step time ended with status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
