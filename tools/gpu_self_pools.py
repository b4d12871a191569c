"""One robot against its own map at demo scale: self loop closures over the device-resident pool (submap_align_pools(p, [pool,
pool]): roman_shared_reduce_dev in front of the batch) against the only way there was for this input before it
(SubmapPool.to_submaps() twice + submap_align_grid: every segment row back to the host as a Python object, packed and uploaded
again; the removal through roman_align_lc_batch_ids).

  python tools/gpu_self_pools.py --out profiles/self_pools/timing.json

Scale: one map driven twice around a 100 m loop (the second lap sees every segment again as a new segment), about 64 submaps of
20-40 objects with 768-d descriptors, method 'roman', no submap descriptor gate (every pair registers).  Both paths run in THIS
process on the same pool after warm-up; wall time from the first enqueue to the results on the host, median of `--reps` each.
No ratio is promised: the numbers are what they are."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 768


def two_lap_map(n_lap, n_poses, dt, loop_radius, seed=8200):
    from roman_amd import synth
    segs, traj, times = synth.make_map(n_lap, D, seed=seed, n_poses=n_poses, loop_radius=loop_radius, laps=1.0, dt=dt)
    rng = np.random.default_rng(seed + 1)
    lap, again = n_poses * dt, []
    for k, s in enumerate(segs):
        q = copy.deepcopy(s)
        q.id = 10 ** 6 + k
        q.centroid = np.asarray(s.centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(s.centroid))
        v = np.asarray(s.semantic_descriptor, dtype=np.float64) + 0.02 * rng.standard_normal(D) / np.sqrt(D)
        q.semantic_descriptor = v / np.linalg.norm(v)
        q.first_seen, q.last_seen = s.first_seen + lap, s.last_seen + lap
        again.append(q)
    return segs + again, list(traj) + [np.array(T) for T in traj], np.concatenate([times, times + lap]), lap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1200, help="segments seen on lap 1")
    ap.add_argument("--poses", type=int, default=640, help="poses per lap")
    ap.add_argument("--loop-radius", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_pools", "timing.json"))
    a = ap.parse_args()
    import torch
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    segs, traj, times, lap = two_lap_map(a.segments, a.poses, 1.0, a.loop_radius)
    p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40,
                          single_robot_lc=True, single_robot_lc_time_thresh=0.9 * lap)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    pool = build_submap_pool(reg, MapTable.from_segments(reg, segs), submap_centers(traj, times, params), params, ctx=ctx, device=dev)

    seen = {}
    reduce_dev = ctx.shared_reduce_dev

    def spy(B, F, feats_ptr, region_row0, *rest):
        seen.update(B=int(B), F=int(F), region_rows=int(np.sum(rest[2], dtype=np.int64) + np.sum(rest[4], dtype=np.int64)))
        return reduce_dev(B, F, feats_ptr, region_row0, *rest)
    ctx.shared_reduce_dev = spy

    def new_way():
        return sa.submap_align_pools(p, [pool, pool], io, registration=reg)

    def old_way():
        return sa.submap_align_grid(p, [pool.to_submaps(segs), pool.to_submaps(segs)], io, registration=reg)

    t = {"pools": [], "grid": []}
    res = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in (("pools", new_way), ("grid", old_way)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res[name] = fn()
            dt = time.perf_counter() - t0
            if rep >= a.warmup:
                t[name].append(dt)
    got, want = res["pools"], res["grid"]
    same = bool(np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True)
                and np.array_equal(got.lc_edges["pairs"], want.lc_edges["pairs"])
                and np.allclose(got.T_ij_hat_mat, want.T_ij_hat_mat, rtol=0, atol=1e-12, equal_nan=True))
    k = pool.nonempty
    sets = [set(pool.ids[s, :pool.count[s]].tolist()) for s in k]
    S = len(k)
    affected = sum(1 for i in range(S) for j in range(S) if sets[i] & sets[j])
    new_ms, old_ms = 1e3 * float(np.median(t["pools"])), 1e3 * float(np.median(t["grid"]))
    out = dict(scale=dict(segments_per_lap=a.segments, d=D, method="roman", submaps=S, objects_min=int(pool.count[k].min()), objects_max=int(pool.count[k].max()),
                          reps=a.reps, warmup=a.warmup),
               problems=seen.get("B"), submap_align_pools_ms=new_ms, to_submaps_plus_submap_align_grid_ms=old_ms, ratio_new_over_old=new_ms / old_ms,
               submap_align_pools_ms_all=[1e3 * x for x in t["pools"]], to_submaps_plus_submap_align_grid_ms_all=[1e3 * x for x in t["grid"]],
               region_bytes=8 * seen.get("F", 0) * seen.get("region_rows", 0), pool_bytes=8 * int(pool.pool.shape[0]) * int(pool.pool.shape[1]),
               share_of_problems_affected=affected / float(S * S), loop_closures=int(len(want.lc_edges["pairs"])), same_results=same)
    ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if same else 2


if __name__ == "__main__":
    sys.exit(main())
