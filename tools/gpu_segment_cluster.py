#!/usr/bin/env python3
"""Times the segment clustering on one MI355X and writes profiles/segment_cluster/timing.json, every
sample kept.  Two cases whose sizes are ASSUMED, as tools/gpu_segment_integrate.py assumes them — nobody here has measured a real
mapper run:
  frame   10 segments going inactive in one frame, 300 ... 3000 points each (log-uniform): a cleaned surface patch at about one
          point per 0.05 m voxel, a satellite patch of a twentieth of its points a metre away and a fiftieth of stray points
  large   one job of 20 000 points of the same make
Without --case this is the driver: every case is a process of its own under its own `timeout`, and the first non-zero exit status
ends the run.  Per case: the device call alone between two events on the context's stream (roman_segment_cluster_dev on resident
clouds), p50 over repeated enqueues after warm-up; the wall time of the host-pointer call; and the CPU oracle's neighbour-list form
(tests/_dbscan_oracle.labels_sequential, NumPy + Python sets on this machine's CPU) on the same clouds, with the check that labels
and kept points agree bit for bit.  The parent has no device path and the reference needs open3d: no ratio to either is claimed."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, REPS = 3, 20
VS, EPS, MIN_POINTS = 0.05, 0.25, 10
CASES = {"frame": 300, "large": 600}          # seconds each case may take


def surface(rng, n, centre, size):
    """n points on a bumpy patch of `size` metres: what a depth camera sees of an object's face"""
    uv = rng.uniform(-0.5, 0.5, (n, 2)) * size
    return centre + np.column_stack([uv, 0.05 * np.sin(6.0 * uv[:, 0]) + 0.01 * rng.normal(size=n)])


def segment(rng, n):
    main, sat = n - n // 20 - n // 50, n // 20
    centre = rng.uniform(-10, 10, 3)
    size = VS * np.sqrt(main) * 0.9
    p = np.vstack([surface(rng, main, centre, size), surface(rng, sat, centre + [size / 2 + 1.0, 0.0, 0.0], VS * np.sqrt(max(sat, 1)) * 0.9),
                   centre + rng.uniform(-1.0, 1.0, (n // 50, 3)) * (size + 2.0)])
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def clouds_of(name):
    rng = np.random.default_rng(6270)
    if name == "frame":
        return [segment(rng, int(np.exp(rng.uniform(np.log(300), np.log(3000))))) for _ in range(10)]
    return [segment(rng, 20000)]


def run_case(name, out):
    import torch
    import _dbscan_oracle as do
    from roman_amd.runtime import Context, cluster_params, cluster_slots
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    clouds = clouds_of(name)
    pts = np.ascontiguousarray(np.vstack(clouds)); off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    jobs = np.arange(len(clouds), dtype=np.int32)
    P = cluster_params(EPS, MIN_POINTS)
    total, nj = int(cluster_slots(off, jobs)[-1]), len(jobs)
    with torch.cuda.stream(stream):
        t_pts, t_off, t_jobs = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(jobs).to(dev)
        o_pts = torch.zeros((total, 3), dtype=torch.float64, device=dev); o_lab = torch.zeros(total, dtype=torch.int32, device=dev)
        o_int = torch.zeros(4 * nj, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        samples = []
        for k in range(WARMUP + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            a.record()                                           # both events on the context's stream: the device alone
            ctx.segment_cluster_dev(P, t_pts.data_ptr(), t_off.data_ptr(), off, t_jobs.data_ptr(), jobs, o_pts.data_ptr(), o_int.data_ptr(),
                                    o_int.data_ptr() + 4 * nj, o_int.data_ptr() + 8 * nj, out_labels_ptr=o_lab.data_ptr(), out_kept_ptr=o_int.data_ptr() + 12 * nj)
            b.record(); b.synchronize()
            if k >= WARMUP:
                samples.append(a.elapsed_time(b))
        e2e = []
        for k in range(1 + 5):
            t0 = time.perf_counter(); r = ctx.segment_cluster(P, pts, off, jobs); e2e.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref = [do.final_cleanup(c, EPS, MIN_POINTS, labels=do.labels_sequential(c, EPS, MIN_POINTS)) for c in clouds]
    oracle_ms = (time.perf_counter() - t0) * 1e3
    labels_equal = all(r.labels(j).tobytes() == x.labels.tobytes() for j, x in enumerate(ref))
    kept_equal = all(r.cloud(j).tobytes() == x.points.tobytes() and r.kept[j] == x.kept for j, x in enumerate(ref))
    n2 = float(sum(len(c) ** 2 for c in clouds))
    case = {"jobs": nj, "points_in": total, "points_kept": int(r.count.sum()), "clusters": r.n_clusters.tolist(),
            "device_ms": samples, "device_ms_p50": float(np.median(samples)), "pairs_per_sweep": n2,
            "segment_cluster_wall_ms": e2e[1:], "cpu_oracle_neighbour_list_ms": oracle_ms,
            "labels_bits_equal_to_oracle": bool(labels_equal), "kept_points_bits_equal_to_oracle": bool(kept_equal)}
    print(name, {k: v for k, v in case.items() if not isinstance(v, list)}, flush=True)
    with open(out, "w") as f:
        json.dump(case, f, indent=1)
    ctx.close()
    return 0 if (labels_equal and kept_equal) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_cluster", "timing.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = {"assumption": "frame: 10 segments of 300-3000 points (log-uniform) going inactive at once; large: one segment of 20000 points; cleaned "
                            "surface patches at about one point per 0.05 m voxel with a satellite patch and stray points; sizes of a real mapper frame "
                            "have not been measured", "eps": EPS, "min_points": MIN_POINTS, "warmup": WARMUP, "reps": REPS, "cases": {}}
    for name, limit in CASES.items():
        part = args.out + f".{name}.part"
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name, "--out", part])
        if rc != 0:
            print(f"case {name} ended with status {rc}: stopping", flush=True)
            return rc
        with open(part) as f:
            result["cases"][name] = json.load(f)
        os.remove(part)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
