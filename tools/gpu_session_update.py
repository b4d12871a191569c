"""A session that grows, step by step: submap_align_session_update against the full submap_align_session
over the same grown pools.

  python tools/gpu_session_update.py --out profiles/session_update/timing.json

Scale: the four robots of tools/gpu_session.py (10^4 segments of 768-d descriptors around a 1 km loop, about 100 submaps each,
method 'roman', 'mean_semantic', the 10 blocks r <= s).  The pools are built once per process at their final size; a step's pools
are their first S_r - K + k submaps (the same pools for both ways).  `update`: per repetition a fresh state, the full first call,
then K steps that append one submap per robot — per step the listed pairs, the TODO pairs registered, the wall time from the call
to the results on the host, and its parts (SessionAlignState.seconds: host block, gate with its uploads and synchronisation,
registration); host + gate is the floor a step pays whatever it lists.  `full`: submap_align_session over each step's pools.
Each way in a process of its own under `timeout -k 10`, 3 warm-up repetitions, 10 timed, every sample kept; the parent starts the
second way only after a clean end of the first and checks that the last step's results agree.  No ratio is promised."""
import argparse
import dataclasses
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT = 540            # seconds per way


def prefix(pool, k):
    """The first k submaps of `pool` as a pool of its own: the session at an earlier step."""
    c = pool.centers
    cen = dataclasses.replace(c, **{f.name: getattr(c, f.name)[:k] for f in dataclasses.fields(c)})
    cut = lambda a, n: None if a is None else a[:n]
    return dataclasses.replace(pool, pool=pool.pool[:k * pool.cap], count=pool.count[:k], src=pool.src[:k], ids=pool.ids[:k], status=pool.status[:k],
                               desc=cut(pool.desc, k), centers=cen, desc_dev=cut(pool.desc_dev, k), ids_dev=cut(pool.ids_dev, k * pool.cap))


def stats(x):
    return dict(seconds_median=float(np.median(x)), seconds_min=float(np.min(x)), seconds_max=float(np.max(x)), seconds=[float(v) for v in x])


def run_way(a, which):
    import gpu_session as gs
    from roman_amd.align import submap_align as sa
    torch, dev, stream, ctx, p, io, reg, final, blocks = gs.setup(a)
    n = [len(q.count) for q in final]
    pools_at = [[prefix(q, m - a.steps + k) for q, m in zip(final, n)] for k in range(a.steps + 1)]
    rows = [dict(step=k, submaps=[int(len(q.nonempty)) for q in pools_at[k]]) for k in range(a.steps + 1)]
    wall, parts = [[] for _ in rows], [[] for _ in rows]
    for rep in range(a.warmup + a.reps):
        state = sa.SessionAlignState()
        for k, pools in enumerate(pools_at):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if which == "update":
                res = sa.submap_align_session_update(state, p, pools, None, blocks, io, registration=reg)
            else:
                res = sa.submap_align_session(p, pools, blocks, io, registration=reg)
            torch.cuda.synchronize(dev)
            if rep >= a.warmup:
                wall[k].append(time.perf_counter() - t0)
                if which == "update":
                    parts[k].append(dict(state.seconds))
            if which == "update":
                rows[k].update(listed_pairs=int(state.listed), all_pairs=int(state.total), registered=int(sum(len(r.timing_list) for r in res.values())))
            else:
                rows[k].update(registered=int(sum(len(r.timing_list) for r in res.values())))
            rows[k]["loop_closures"] = int(sum(len(r.lc_edges["pairs"]) for r in res.values()))
    for k, row in enumerate(rows):
        row.update(stats(wall[k]))
        if which == "update":
            for name in ("host", "gate", "register"):
                row[name + "_seconds_median"] = float(np.median([q.get(name, 0.0) for q in parts[k]]))
            row["floor_seconds_median"] = row["host_seconds_median"] + row["gate_seconds_median"]
    np.savez(a.dump, **gs.summary(res, blocks))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--way", default=None, choices=["update", "full"], help="(internal) run one way in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--steps", type=int, default=4, help="appending steps behind the full first call")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8)
    ap.add_argument("--skip", type=float, default=float("inf"))
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_update", "timing.json"))
    a = ap.parse_args()
    if a.way:
        print("WAY_JSON " + json.dumps(run_way(a, a.way)))
        return 0
    out = dict(scale=dict(robots=a.robots, segments=a.segments, d=768, method="roman", submap_descriptor="mean_semantic", thresh=a.thresh, steps=a.steps,
                          reps=a.reps, warmup=a.warmup))
    dumps = {}
    with tempfile.TemporaryDirectory() as td:
        for way in ("update", "full"):
            dumps[way] = os.path.join(td, way + ".npz")
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--way", way, "--dump", dumps[way]] + \
                  [x for k in ("steps", "robots", "segments", "reps", "warmup", "thresh", "skip") for x in ("--" + k, str(getattr(a, k)))] + \
                  ["--time-thresh", str(a.time_thresh)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("WAY_JSON ")]
            if r.returncode != 0 or not line:                # nothing more is started on the device after a step that did not end clean
                print(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode or 1
            out[way] = json.loads(line[0][len("WAY_JSON "):])
        za, zb = np.load(dumps["update"]), np.load(dumps["full"])
        out["same_results_at_the_last_step"] = bool(sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    for u, w in zip(out["update"], out["full"]):
        print(f"step {u['step']}: listed {u['listed_pairs']} of {u['all_pairs']} pairs, registered {u['registered']} (full: {w['registered']}), "
              f"update {1e3 * u['seconds_median']:.1f} ms (floor {1e3 * u['floor_seconds_median']:.1f} ms), full call {1e3 * w['seconds_median']:.1f} ms")
    print("same results at the last step:", out["same_results_at_the_last_step"])
    return 0 if out["same_results_at_the_last_step"] else 1


if __name__ == "__main__":
    sys.exit(main())
