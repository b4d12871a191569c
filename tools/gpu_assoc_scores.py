#!/usr/bin/env python3
"""Times the frame data association scores on one MI355X and writes profiles/assoc_scores/timing.json,
every sample kept.  Two cases whose sizes are ASSUMED — nobody here has measured a real mapper run:
  frame   300 segments of 50 ... 2000 points (log-uniform) against 40 observations of 500 ... 20 000 points, d = 768 descriptors,
          cosine as second criterion; segments spread over 40 m x 40 m, an observation lies on one of them: most pairs disjoint
  merge   the 300 segments against themselves (self mode), IoM, one criterion
Per case: the device call alone between two events on the context's stream (roman_assoc_scores_dev on resident clouds, warm
caches), the wall time of association_scores end to end (stacking, upload, call, read-back), and the literal loop of the NumPy
oracle (tests/_voxel_oracle.literal_scores: the reference's dense arrays and slices per pair, grids built once per cloud as the
reference caches them) on this machine's CPU, with the check that both give the same geo bits.  The reference itself needs
open3d and runs on neither machine; no ratio to it is claimed.  A sweep over the two path cuts (roman_ctx_set_assoc_cuts)
records where one path starts to beat the other."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, REPS = 3, 20


def make_clouds(points_list, desc=None):
    from roman_amd.align import SegmentClouds
    off = np.zeros(len(points_list) + 1, dtype=np.int64); off[1:] = np.cumsum([len(p) for p in points_list])
    n = len(points_list)
    return SegmentClouds(np.ascontiguousarray(np.vstack(points_list)), off, np.arange(n, dtype=np.int64), np.zeros((n, 2)), desc)


def frame_scene(rng, n_seg=300, n_obs=40, d=768):
    centres = np.column_stack([rng.uniform(-20.0, 20.0, (n_seg, 2)), rng.uniform(0.0, 2.0, n_seg)])
    counts = np.exp(rng.uniform(np.log(50), np.log(2000), n_seg)).astype(np.int64)
    segs = [c + rng.normal(size=(int(n), 3)) * rng.uniform(0.2, 0.8, 3) for c, n in zip(centres, counts)]
    seen = rng.choice(n_seg, n_obs, replace=False)
    ocounts = np.exp(rng.uniform(np.log(500), np.log(20000), n_obs)).astype(np.int64)
    obs = [centres[s] + rng.normal(size=3) * 0.05 + rng.normal(size=(int(n), 3)) * rng.uniform(0.2, 0.8, 3) for s, n in zip(seen, ocounts)]
    ds = rng.normal(size=(n_seg, d)); ds /= np.linalg.norm(ds, axis=1, keepdims=True)
    do = ds[seen] + 0.02 * rng.normal(size=(n_obs, d))
    return segs, obs, ds, do


def device_ms(torch, ctx, aparams, pts, off, N1, N2, desc, reps=REPS):
    dev = torch.device("cuda:0")
    cols = N1 if N2 < 0 else N2
    clouds = len(off) - 1
    t_pts, t_off = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    t_desc = torch.from_numpy(desc).to(dev) if desc is not None else None
    f = torch.zeros((3, N1, cols), dtype=torch.float64, device=dev); i = torch.zeros(N1 * cols + 2 * clouds, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    samples = []
    for k in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.sync()
        a.record()                                               # both events on the context's stream: the device alone
        ctx.assoc_scores_dev(aparams, t_pts.data_ptr(), t_off.data_ptr(), off, N1, N2, t_desc.data_ptr() if desc is not None else None,
                             0 if desc is None else desc.shape[1], f[0].data_ptr(), f[2].data_ptr(), i.data_ptr() + 4 * (N1 * cols + clouds),
                             sem_ptr=f[1].data_ptr() if aparams.semantic else None, inter_ptr=i.data_ptr(), n_vox_ptr=i.data_ptr() + 4 * N1 * cols)
        b.record(); b.synchronize()
        if k >= WARMUP:
            samples.append(a.elapsed_time(b))
    return samples, f[0].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_scores", "timing.json"))
    args = ap.parse_args()
    import torch
    import _voxel_oracle as vo
    from roman_amd.map import AssociationParams, association_scores
    from roman_amd.map.association import _stacked
    from roman_amd.runtime import Context
    stream = torch.cuda.Stream(torch.device("cuda:0")); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(6250)
    segs, obs, ds, do = frame_scene(rng)
    result = {"assumption": "300 segments of 50-2000 points (log-uniform), 40 observations of 500-20000 points, d = 768, segments spread over "
                            "40 m x 40 m and every observation on one of them: sizes of a real mapper frame have not been measured",
              "voxel_size": 0.2, "cases": {}}
    cases = {"frame": (make_clouds(segs, ds), make_clouds(obs, do), AssociationParams(semantic_association_method="cosine_similarity"),
                       vo.params(0.2, "iou", True), (segs, obs, ds, do)),
             "merge": (make_clouds(segs), None, AssociationParams(geometric_association_method="iom"), vo.params(0.2, "iom"), (segs, None, None, None))}
    with torch.cuda.stream(stream):
        for name, (ca, cb, P, op, lit) in cases.items():
            aparams, pts, off, N1, N2, desc = _stacked(ca, cb, P)
            ms, geo = device_ms(torch, ctx, aparams, pts, off, N1, N2, desc)
            e2e = []
            for k in range(1 + 5):
                t0 = time.perf_counter(); r = association_scores(ca, cb, P, ctx=ctx); e2e.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            geo_l, _ = vo.literal_scores(lit[0], lit[1], op, lit[2], lit[3])
            loop_ms = (time.perf_counter() - t0) * 1e3
            case = {"rows": N1, "cols": N1 if N2 < 0 else N2, "points": int(off[-1]), "voxels": int(r.n_vox.sum()), "pairs_with_intersection": int(np.count_nonzero(r.inter)),
                    "device_ms": ms, "device_ms_median": float(np.median(ms)), "association_scores_wall_ms": e2e[1:],
                    "numpy_literal_loop_ms": loop_ms, "geo_bits_equal_to_literal_loop": bool(geo_l.tobytes() == geo.tobytes() == r.geo.tobytes())}
            result["cases"][name] = case
            print(name, {k: v for k, v in case.items() if not isinstance(v, list)}, flush=True)
        # the two cuts: 2000 clouds of n points each against one column of one point, every cloud forced down either path
        aparams = AssociationParams().abi()
        sweep = {"wave_vs_lds_workgroup": {}, "lds_workgroup_vs_merge": {}}
        for n in (32, 64, 128, 256, 512):
            pl = [c + rng.normal(size=(n, 3)) * 0.5 for c in rng.uniform(-20, 20, (2000, 3))] + [np.zeros((1, 3))]
            pts = np.ascontiguousarray(np.vstack(pl)); off = np.concatenate([[0], np.cumsum([len(p) for p in pl])]).astype(np.int64)
            row = {}
            for path, cuts in (("wave", (512, 0)), ("lds_workgroup", (1, 0))):
                ctx.set_assoc_cuts(*cuts)
                row[path] = device_ms(torch, ctx, aparams, pts, off, 2000, 1, None, reps=10)[0]
            ctx.set_assoc_cuts(0, 0)
            sweep["wave_vs_lds_workgroup"][str(n)] = row
            print("cut", n, {p: float(np.median(v)) for p, v in row.items()}, flush=True)
        for n in (1024, 2048, 4096, 8192):
            pl = [c + rng.normal(size=(n, 3)) * 0.8 for c in rng.uniform(-20, 20, (500, 3))] + [np.zeros((1, 3))]
            pts = np.ascontiguousarray(np.vstack(pl)); off = np.concatenate([[0], np.cumsum([len(p) for p in pl])]).astype(np.int64)
            row = {}
            for path, cuts in (("lds_workgroup", (64, 0)), ("merge_two_chunks", (64, n // 2)), ("merge_four_chunks", (64, n // 4))):
                ctx.set_assoc_cuts(*cuts)
                row[path] = device_ms(torch, ctx, aparams, pts, off, 500, 1, None, reps=10)[0]
            ctx.set_assoc_cuts(0, 0)
            sweep["lds_workgroup_vs_merge"][str(n)] = row
            print("cut", n, {p: float(np.median(v)) for p, v in row.items()}, flush=True)
        result["cut_sweep"] = sweep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
