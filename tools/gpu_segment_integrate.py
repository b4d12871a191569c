#!/usr/bin/env python3
"""Times the segment update on one MI355X and writes profiles/segment_integrate/timing.json, every
sample kept.  Two cases whose sizes are ASSUMED — nobody here has measured a real mapper run:
  frame   40 jobs at voxel size 0.05 m: 30 segments of 300 ... 3000 points (log-uniform) each updated with a posed observation of
          half to twice its size on the same surface, and 10 new segments
  large   one job: a segment of 20 000 points with an observation of 10 000
Per case: the device call alone between two events on the context's stream (roman_segment_integrate_dev on resident clouds),
with and without the outlier step, the wall time of the host-pointer call end to end, and the NumPy oracle on this machine's
CPU with the check that counts and kept points agree.  The parent has no device path and the reference needs open3d: no ratio
is claimed; the numbers are a baseline for later work."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, REPS = 3, 20
VS = 0.05


def surface(rng, n, centre, size):
    """n points on a bumpy patch of `size` metres: what a depth camera sees of an object's face"""
    uv = rng.uniform(-0.5, 0.5, (n, 2)) * size
    return centre + np.column_stack([uv, 0.05 * np.sin(6.0 * uv[:, 0]) + 0.01 * rng.normal(size=n)])


def pose(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4); T[:3, :3] = q * np.sign(np.linalg.det(q)); T[:3, 3] = rng.normal(size=3)
    return T


def frame_case(rng, n_upd=30, n_new=10):
    clouds, jobs, poses = [], [], []
    for _ in range(n_upd):
        n = int(np.exp(rng.uniform(np.log(300), np.log(3000))))
        centre, size = rng.uniform(-10, 10, 3), VS * np.sqrt(n) * 0.9          # about one point per voxel: a cloud that was cleaned before
        T = pose(rng)
        clouds += [surface(rng, n, centre, size), (surface(rng, int(n * rng.uniform(0.5, 2.0)), centre, size) - T[:3, 3]) @ T[:3, :3]]
        jobs.append((len(clouds) - 2, len(clouds) - 1, len(poses))); poses.append(T)
    for _ in range(n_new):
        n = int(np.exp(rng.uniform(np.log(300), np.log(3000))))
        T = pose(rng)
        clouds.append((surface(rng, n, rng.uniform(-10, 10, 3), VS * np.sqrt(n) * 0.5) - T[:3, 3]) @ T[:3, :3])
        jobs.append((None, len(clouds) - 1, len(poses))); poses.append(T)
    return clouds, jobs, np.array(poses)


def large_case(rng):
    T = pose(rng)
    centre, size = np.zeros(3), VS * np.sqrt(20000) * 0.9
    return [surface(rng, 20000, centre, size), (surface(rng, 10000, centre, size) - T[:3, 3]) @ T[:3, :3]], [(0, 1, 0)], np.array([T])


def device_ms(torch, ctx, iparams, pts, off, jobs, poses, reps=REPS):
    from roman_amd.runtime import integrate_jobs, integrate_slots
    dev = torch.device("cuda:0")
    table = integrate_jobs(jobs)
    total, n_jobs = int(integrate_slots(off, table)[-1]), len(table)
    t_pts, t_off, t_pose = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(poses).to(dev)
    t_jobs = torch.from_numpy(table.view(np.int32).reshape(-1, 3).copy()).to(dev)
    out = torch.zeros((total, 3), dtype=torch.float64, device=dev); ci = torch.zeros(2 * n_jobs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    samples = []
    for k in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.sync()
        a.record()                                               # both events on the context's stream: the device alone
        ctx.segment_integrate_dev(iparams, t_pts.data_ptr(), t_off.data_ptr(), off, t_pose.data_ptr(), len(poses), t_jobs.data_ptr(), table,
                                  out.data_ptr(), ci.data_ptr(), ci.data_ptr() + 4 * n_jobs)
        b.record(); b.synchronize()
        if k >= WARMUP:
            samples.append(a.elapsed_time(b))
    return samples, ci[:n_jobs].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_integrate", "timing.json"))
    args = ap.parse_args()
    import torch
    import _integrate_oracle as io
    from roman_amd.runtime import Context, integrate_params
    stream = torch.cuda.Stream(torch.device("cuda:0")); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(6260)
    result = {"assumption": "frame: 30 segments of 300-3000 points (log-uniform) each with a posed observation of 0.5-2 times its size on the same "
                            "surface, and 10 new segments; large: 20000 + 10000 points; sizes of a real mapper frame have not been measured",
              "voxel_size": VS, "cases": {}}
    with torch.cuda.stream(stream):
        for name, (clouds, jobs, poses) in (("frame", frame_case(rng)), ("large", large_case(rng))):
            pts = np.ascontiguousarray(np.vstack(clouds)); off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
            on, off_p = integrate_params(VS, 1.0), integrate_params(VS, None)
            ms_on, count = device_ms(torch, ctx, on, pts, off, jobs, poses)
            ms_off, down = device_ms(torch, ctx, off_p, pts, off, jobs, poses)
            e2e = []
            for k in range(1 + 5):
                t0 = time.perf_counter(); r = ctx.segment_integrate(on, pts, off, jobs, poses); e2e.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ref = [io.integrate(None if b is None else clouds[b], clouds[a], poses[p], io.params(VS, 1.0)) for b, a, p in jobs]
            oracle_ms = (time.perf_counter() - t0) * 1e3
            agree = all(len(x.down) == d and len(x.points) == c for x, d, c in zip(ref, down, count))
            exact = all(r.cloud(j).tobytes() == x.points.tobytes() for j, x in enumerate(ref))
            case = {"jobs": len(jobs), "points_in": int(sum(len(clouds[a]) + (0 if b is None else len(clouds[b])) for b, a, _ in jobs)),
                    "points_down_sampled": int(down.sum()), "points_kept": int(count.sum()),
                    "device_ms": ms_on, "device_ms_median": float(np.median(ms_on)),
                    "device_ms_without_outlier_step": ms_off, "device_ms_without_outlier_step_median": float(np.median(ms_off)),
                    "segment_integrate_wall_ms": e2e[1:], "numpy_oracle_ms": oracle_ms,
                    "counts_agree_with_oracle": bool(agree), "kept_points_bits_equal_to_oracle": bool(exact)}
            result["cases"][name] = case
            print(name, {k: v for k, v in case.items() if not isinstance(v, list)}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
