"""The pools of a session that grows, step by step: grow_session_pools against build_session_pools over the
same step's inputs.

  python tools/gpu_session_grow.py --out profiles/session_grow/timing.json

Scale: the four maps of tools/gpu_session_submaps.py (10^4 segments with 768-d descriptors around a 1 km loop, about 100 submap
centres each, at most 40 segments per submap, 'mean_semantic'), their rows in the order of first sight.  A stage holds, per robot,
the centres but the last K - k and the rows first seen up to the stage's last pose: a step appends one submap and a few rows per
robot and moves the former last submap's t_hi.  --center-time (SubmapParams.time_threshold) is finite: with an infinite window every
appended row passes every old submap's time test and the list rule of §4.21 names every submap.
`grow`: per repetition a fresh state, the first call over stage 0, then K steps — per step the wall time of grow_session_pools from
the call to the pools, its parts (SessionPoolsState.seconds: upload — host rules, moves, table rows —, device, read-back) and the
submaps listed and touched.  `full`: build_session_pools over each stage's inputs; --full-root names a checkout of another commit (the
parent's) whose package that process imports instead.  Each way in a process of its own under `timeout -k 10`, 3 warm-up
repetitions, 10 timed, every sample kept; the parent process starts the second way only after a clean end of the first and checks
that the last stage's pools agree byte for byte.  No ratio is promised."""
import argparse
import dataclasses
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 540            # seconds per way


def stages_of(a, params, tables, centers, trajs):
    """-> list over stages of (tables, centers)"""
    from roman_amd.align.submaps import submap_centers
    out = []
    for k in range(a.steps + 1):
        tb, cn = [], []
        for t, c, (traj, times) in zip(tables, centers, trajs):
            back = a.steps - k
            poses = len(times) if back == 0 else int(c.index[len(c) - back])
            n = len(t) if back == 0 else int(np.searchsorted(t.times[:, 0], times[poses - 1], side="right"))
            tb.append(dataclasses.replace(t, feats=t.feats[:n], times=t.times[:n], ids=t.ids[:n]))
            cn.append(submap_centers(traj[:poses], times[:poses], params))
        out.append((tb, cn))
    return out


def digest(pools):
    h = hashlib.sha256()
    for q in pools:
        for x in (q.pool.cpu().numpy(), q.count, q.src, q.ids, q.status, q.desc):
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def stats(x):
    return dict(seconds_median=float(np.median(x)), seconds_min=float(np.min(x)), seconds_max=float(np.max(x)), seconds=[float(v) for v in x])


def run_way(a, which):
    sys.path.insert(0, os.path.abspath(a.full_root) if which == "full" and a.full_root else ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import gpu_session_submaps as gs
    from roman_amd import synth
    from roman_amd.align import submaps as sm
    torch, dev, stream, ctx, p, io, reg, params, tables, centers, blocks = gs.setup(a)
    params = dataclasses.replace(params, time_threshold=a.center_time)
    _, traj, times = synth.make_map(a.segments, gs.D, seed=8100, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
    trajs = [(traj[40 * r:], np.asarray(times[40 * r:], dtype=np.float64)) for r in range(a.robots)]
    order = [np.argsort(t.times[:, 0], kind="stable") for t in tables]      # rows in the order of first sight: a step appends the recent ones
    tables = [dataclasses.replace(t, feats=np.ascontiguousarray(t.feats[o]), times=np.ascontiguousarray(t.times[o]), ids=np.ascontiguousarray(t.ids[o]))
              for t, o in zip(tables, order)]
    centers = [sm.submap_centers(tr, tm, params) for tr, tm in trajs]
    stages = stages_of(a, params, tables, centers, trajs)
    rows = [dict(step=k, segments=[len(t) for t in tb], submaps=[len(c) for c in cn]) for k, (tb, cn) in enumerate(stages)]
    wall, parts = [[] for _ in rows], [[] for _ in rows]
    for rep in range(a.warmup + a.reps):
        state = None
        for k, (tb, cn) in enumerate(stages):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if which == "grow":
                pools, touched, state = sm.grow_session_pools(state, reg, tb, cn, params, ctx=ctx, device=dev)
            else:
                pools = sm.build_session_pools(reg, tb, cn, params, ctx=ctx, device=dev)
            torch.cuda.synchronize(dev)
            if rep >= a.warmup:
                wall[k].append(time.perf_counter() - t0)
                if which == "grow":
                    parts[k].append(dict(state.seconds))
            if which == "grow":
                rows[k].update(listed=int(state.listed), total=int(state.total), touched=int(sum(int(t.sum()) for t in touched)))
    for k, row in enumerate(rows):
        row.update(stats(wall[k]))
        if which == "grow":
            for name in ("upload", "device", "readback"):
                row[name + "_seconds_median"] = float(np.median([q[name] for q in parts[k]]))
                row[name + "_seconds"] = [float(q[name]) for q in parts[k]]
    out = dict(steps=rows, digest_of_the_last_stage=digest(pools))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--way", default=None, choices=["grow", "full"], help="(internal) run one way in this process")
    ap.add_argument("--full-root", dest="full_root", default=None, help="a checkout whose roman_amd the `full` way imports (the parent commit's)")
    ap.add_argument("--steps", type=int, default=4, help="appending steps behind the first call")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--center-time", dest="center_time", type=float, default=30.0, help="SubmapParams.time_threshold, seconds")
    ap.add_argument("--thresh", type=float, default=0.8)
    ap.add_argument("--skip", type=float, default=float("inf"))
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_grow", "timing.json"))
    a = ap.parse_args()
    if a.way:
        print("WAY_JSON " + json.dumps(run_way(a, a.way)))
        return 0
    out = dict(scale=dict(robots=a.robots, segments=a.segments, d=768, submap_descriptor="mean_semantic", steps=a.steps, center_time=a.center_time,
                          reps=a.reps, warmup=a.warmup, full_root_given=bool(a.full_root)))
    for way in ("grow", "full"):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--way", way] + \
              [x for k in ("steps", "robots", "segments", "reps", "warmup", "thresh", "skip") for x in ("--" + k, str(getattr(a, k)))] + \
              ["--time-thresh", str(a.time_thresh), "--center-time", str(a.center_time)] + (["--full-root", a.full_root] if a.full_root else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("WAY_JSON ")]
        if r.returncode != 0 or not line:                    # nothing more is started on the device after a way that did not end clean
            print(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode or 1
        out[way] = json.loads(line[0][len("WAY_JSON "):])
    out["same_pools_at_the_last_stage"] = out["grow"]["digest_of_the_last_stage"] == out["full"]["digest_of_the_last_stage"]
    for u, w in zip(out["grow"]["steps"], out["full"]["steps"]):
        u["full_over_grow"] = w["seconds_median"] / u["seconds_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    for u, w in zip(out["grow"]["steps"], out["full"]["steps"]):
        print(f"step {u['step']}: {sum(u['submaps'])} submaps, listed {u['listed']}, touched {u['touched']}; grow {1e3 * u['seconds_median']:.2f} ms "
              f"({1e3 * u['seconds_min']:.2f} - {1e3 * u['seconds_max']:.2f}; upload {1e3 * u['upload_seconds_median']:.2f}, device {1e3 * u['device_seconds_median']:.2f}, "
              f"read-back {1e3 * u['readback_seconds_median']:.2f}), full build {1e3 * w['seconds_median']:.2f} ms ({1e3 * w['seconds_min']:.2f} - {1e3 * w['seconds_max']:.2f})")
    print("same pools at the last stage:", out["same_pools_at_the_last_stage"])
    return 0 if out["same_pools_at_the_last_stage"] else 1


if __name__ == "__main__":
    sys.exit(main())
