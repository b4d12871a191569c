"""Force-fill submaps and the bounding-box gate at demo scale: two maps cut into 64 force-fill submaps each
(max_size 40, overlap 20: slices of 20-40 objects, 768-d descriptors, method 'roman'), pass 1 of the 64 x 64 grid in AABB mode.

  python tools/gpu_fill_boxes.py --out profiles/fill_boxes/timing.json

Two ways to the list of the pairs to register, in THIS process, the median of `--reps` runs after `--warmup`:
  device_resident_path   build_submap_pool(fill=...) x 2 (roman_submaps_fill_dev), roman_submap_boxes_dev x 2, roman_grid_gate_aabb_dev,
                         n_todo and the pair list back on the host.  Events on the context's stream bracket it (they span the
                         host work between the enqueues too); wall time beside them.
  host_submaps_path      what this input took before: the same pools, SubmapPool.to_submaps() x 2, then submap_align_grid until
                         it enters its batched call — pass 1 in NumPy with the boxes in a Python loop over submaps, and the
                         packing of the registered submaps for the upload (that path has no earlier point at which the list exists).
The two TODO lists are compared.  No ratio is promised: first measurements, the numbers are what they are."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 768


class _Stop(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--submaps", type=int, default=64)
    ap.add_argument("--max-size", type=int, default=40)
    ap.add_argument("--overlap", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_boxes", "timing.json"))
    a = ap.parse_args()
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import FillSubmapParams, MapTable, build_submap_pool, fill_centers
    from roman_amd.runtime import Context, grid_gate_params
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="roman", semantics_dim=D, force_fill_submaps=True, submap_max_size=a.max_size, submap_overlap=a.overlap)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = p.get_object_registration(); reg.set_context(ctx)
    fp = FillSubmapParams.from_submap_align_params(p)
    n_seg = a.submaps * (a.max_size - a.overlap)
    maps = []
    for r in range(2):                                         # the same place mapped twice: cross pairs have true matches
        segs, traj, times = synth.make_map(n_seg, D, seed=8300, n_poses=640, loop_radius=50.0, laps=1.3, dt=1.0)
        for q in segs:
            q.id = int(q.id) + 10 ** 6 * r
        maps.append((segs, traj, times, MapTable.from_segments(reg, segs)))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def build():
        pools = []
        for _, traj, times, table in maps:
            centers, slices = fill_centers(table, traj, times, fp)
            pools.append(build_submap_pool(reg, table, centers, fp, ctx=ctx, device=dev, fill=slices))
        return pools

    def device_path():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter(); e0.record(stream)
        pools = build()
        n = [len(q.count) for q in pools]                        # (every force-fill slice holds a segment: no submap is dropped)
        B = n[0] * n[1]
        side = [dict(pos=up(q.centers.pose_flu[:, :3, 3]), T=up(q.centers.pose_flu.reshape(-1, 16)), time=up(q.centers.time), cnt=up(q.count),
                     box=torch.empty((len(q.count), 6), dtype=torch.float64, device=dev)) for q in pools]
        f64, i32 = torch.float64, torch.int32
        o = [torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=f64, device=dev),
             torch.empty(16 * B, dtype=f64, device=dev), torch.empty(2 * B, dtype=i32, device=dev), torch.empty(16 * B, dtype=f64, device=dev),
             torch.empty(B, dtype=i32, device=dev), torch.zeros(1, dtype=i32, device=dev)]
        stream.synchronize()
        for q, s in zip(pools, side):
            ctx.submap_boxes_dev(len(q.count), int(q.pool.shape[1]), q.cap, q.pool.data_ptr(), s["cnt"].data_ptr(), s["T"].data_ptr(), s["box"].data_ptr())
        ctx.grid_gate_aabb_dev(grid_gate_params(None, io.skip_distance), n[0], n[1], side[0]["pos"].data_ptr(), side[0]["T"].data_ptr(), side[1]["pos"].data_ptr(),
                               side[1]["T"].data_ptr(), *[t.data_ptr() for t in o], box0_ptr=side[0]["box"].data_ptr(), box1_ptr=side[1]["box"].data_ptr(),
                               time0_ptr=side[0]["time"].data_ptr(), time1_ptr=side[1]["time"].data_ptr())
        e1.record(stream)
        ctx.sync()
        n_todo = int(o[8].cpu().numpy()[0])
        pairs = o[5].cpu().numpy().reshape(-1, 2)[:n_todo].copy()
        t1 = time.perf_counter(); e1.synchronize()
        nearby = (o[1].cpu().numpy().reshape(n) & 1) != 0
        return dict(wall_ms=1e3 * (t1 - t0), event_ms=float(e0.elapsed_time(e1))), pairs, nearby, n

    def host_path():
        seen = {}

        def compute(registration, batch, lc):
            seen["t"] = time.perf_counter(); seen["pairs"] = np.array(batch.pair_index)
            raise _Stop()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pools = build()
        t1 = time.perf_counter()
        subs = [q.to_submaps(m[0]) for q, m in zip(pools, maps)]
        t2 = time.perf_counter()
        try:
            sa.submap_align_grid(p, subs, io, registration=reg, compute=compute)
        except _Stop:
            pass
        return dict(wall_ms=1e3 * (seen["t"] - t0), build_pools_ms=1e3 * (t1 - t0), to_submaps_ms=1e3 * (t2 - t1), pass1_and_packing_ms=1e3 * (seen["t"] - t2)), seen["pairs"]

    dev_runs, host_runs = [], []
    for rep in range(a.warmup + a.reps):
        d_, pairs_d, nearby, n = device_path()
        h_, pairs_h = host_path()
        if rep >= a.warmup:
            dev_runs.append(d_); host_runs.append(h_)
    med = lambda runs: {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    out = dict(scale=dict(grid=n, max_size=a.max_size, overlap=a.overlap, segments_per_map=n_seg, d=D, method="roman", reps=a.reps, warmup=a.warmup),
               device_resident_path=med(dev_runs), host_submaps_path=med(host_runs), n_todo=int(len(pairs_d)), nearby=int(nearby.sum()),
               same_todo_list=bool(np.array_equal(pairs_d, pairs_h)))
    ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if out["same_todo_list"] else 2


if __name__ == "__main__":
    sys.exit(main())
