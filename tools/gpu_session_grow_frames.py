"""The pools of a growing session in the frame-descriptor modes, step by step: grow_session_pools of this
commit against grow_session_pools of the parent commit over the same inputs.

  python tools/gpu_session_grow_frames.py --parent-root <checkout of the parent commit, built> --out profiles/session_grow_frames/timing.json

Scale: the session of tools/gpu_session_grow.py (four maps of 10^4 segments around a 1 km loop, about 100 submap centres each, rows in
the order of first sight, a finite centre time window), with one frame per pose and 768-d frame descriptors; a stage holds the frames
up to its last pose, so a step appends frames at the end.  Both modes: 'mean_frame_descriptor' and 'stacked_frame_descriptors' (with
--frame-dist).  Each (mode, side) in a process of its own under `timeout -k 10`: per repetition a fresh state, the first call over
stage 0, then the steps — per step the wall time of grow_session_pools, its parts (SessionPoolsState.seconds), the frame bytes that
went up (this commit: the appended frames; the parent: every robot's table) and the slots reselected of the total.  3 warm-up
repetitions, 10 timed, every sample kept.  The parent is the baseline, never this code; nothing more is started on the device after
a side that did not end clean; the last stage's pools of the two sides must agree byte for byte.  A second run with another --out (§6.23: timing_repeat.json) gives the run-to-run spread.  No ratio is
promised."""
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
LIMIT = 500            # seconds per (mode, side)
MODES = ("mean_frame_descriptor", "stacked_frame_descriptors")


def digest(pools):
    h = hashlib.sha256()
    for q in pools:
        for x in (q.pool.cpu().numpy(), q.count, q.src, q.ids, q.status, q.frame_n, q.frame_mask.cpu().numpy()) + ((q.desc,) if q.desc is not None else ()):
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def run_side(a):
    root = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_session_grow as gg
    import gpu_session_submaps as gs                                         # (puts this tree in front of sys.path as it is imported ...
    sys.path.insert(0, root)                                                 # ... so the side's own root goes in front of that, before roman_amd is imported)
    import roman_amd
    from roman_amd import synth
    from roman_amd.align import submaps as sm
    if os.path.dirname(os.path.dirname(os.path.abspath(roman_amd.__file__))) != root:
        raise SystemExit(f"roman_amd came from {roman_amd.__file__}, not from {root}: the sides would measure one tree twice")
    torch, dev, stream, ctx, p, io, reg, params, tables, centers, blocks = gs.setup(a)
    params = dataclasses.replace(params, time_threshold=a.center_time, submap_descriptor=a.mode,
                                 frame_descriptor_dist=a.frame_dist if a.mode == "stacked_frame_descriptors" else None)
    _, traj, times = synth.make_map(a.segments, gs.D, seed=8100, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
    trajs = [(traj[40 * r:], np.asarray(times[40 * r:], dtype=np.float64)) for r in range(a.robots)]
    order = [np.argsort(t.times[:, 0], kind="stable") for t in tables]
    tables = [dataclasses.replace(t, feats=np.ascontiguousarray(t.feats[o]), times=np.ascontiguousarray(t.times[o]), ids=np.ascontiguousarray(t.ids[o]))
              for t, o in zip(tables, order)]
    centers = [sm.submap_centers(tr, tm, params) for tr, tm in trajs]
    stages = gg.stages_of(a, params, tables, centers, trajs)
    rng = np.random.default_rng(77)
    full = [sm.FrameTable.from_map(tr, tm, rng.standard_normal((len(tm), gs.D))) for tr, tm in trajs]
    frames = []
    for k in range(a.steps + 1):
        back = a.steps - k
        n = [len(tm) if back == 0 else int(c.index[len(c) - back]) for c, (_, tm) in zip(centers, trajs)]
        frames.append([sm.FrameTable(f.times[:m], f.pos[:m], f.desc[:m]) for f, m in zip(full, n)])
    per_frame = 8 * (1 + 3 + gs.D)
    rows = [dict(step=k, submaps=[len(c) for c in cn], frames=[len(f) for f in fr]) for k, ((tb, cn), fr) in enumerate(zip(stages, frames))]
    wall, parts = [[] for _ in rows], [[] for _ in rows]
    for rep in range(a.warmup + a.reps):
        state = None
        for k, ((tb, cn), fr) in enumerate(zip(stages, frames)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            pools, touched, state = sm.grow_session_pools(state, reg, tb, cn, params, ctx=ctx, device=dev, frames=fr)
            torch.cuda.synchronize(dev)
            if rep >= a.warmup:
                wall[k].append(time.perf_counter() - t0)
                parts[k].append(dict(state.seconds))
            up = getattr(state, "frames_uploaded", None)             # (the parent uploads every table and reselects every slot)
            rows[k].update(rebuilt=int(state.listed), total=int(state.total), touched=int(sum(int(t.sum()) for t in touched)),
                           frame_bytes_uploaded=per_frame * int(sum(len(f) for f in fr) if up is None else up),
                           reselected=int(getattr(state, "frames_listed", state.total)))
    for k, row in enumerate(rows):
        row.update(seconds_median=float(np.median(wall[k])), seconds_min=float(np.min(wall[k])), seconds_max=float(np.max(wall[k])),
                   seconds=[float(v) for v in wall[k]])
        for name in ("upload", "device", "readback"):
            row[name + "_seconds_median"] = float(np.median([q[name] for q in parts[k]]))
            row[name + "_seconds"] = [float(q[name]) for q in parts[k]]
    out = dict(steps=rows, digest_of_the_last_stage=digest(pools), package=os.path.relpath(os.path.dirname(roman_amd.__file__), ROOT),
               context_selects_by_list=hasattr(ctx, "session_frame_select_list_dev"))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", default=None, choices=["this", "parent"], help="(internal) run one side in this process")
    ap.add_argument("--mode", default=None, choices=MODES, help="(internal) the side's submap_descriptor")
    ap.add_argument("--root", default=None, help="(internal) the checkout whose roman_amd the side imports")
    ap.add_argument("--parent-root", dest="parent_root", default=None, help="a built checkout of the parent commit: the baseline")
    ap.add_argument("--steps", type=int, default=4, help="appending steps behind the first call")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--center-time", dest="center_time", type=float, default=30.0, help="SubmapParams.time_threshold, seconds")
    ap.add_argument("--frame-dist", dest="frame_dist", type=float, default=2.0, help="frame_descriptor_dist of the stacked mode, metres")
    ap.add_argument("--thresh", type=float, default=0.8)
    ap.add_argument("--skip", type=float, default=float("inf"))
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_grow_frames", "timing.json"))
    a = ap.parse_args()
    if a.side:
        print("SIDE_JSON " + json.dumps(run_side(a)))
        return 0
    if not a.parent_root:
        print("--parent-root is needed: the parent commit is the baseline")
        return 2
    out = dict(scale=dict(robots=a.robots, segments=a.segments, d=768, steps=a.steps, center_time=a.center_time, frame_dist=a.frame_dist, reps=a.reps, warmup=a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ok = True
    for mode in MODES:
        out[mode] = {}
        for side, root in (("parent", a.parent_root), ("this", ROOT)):
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--side", side, "--mode", mode, "--root", root] + \
                  [x for k in ("steps", "robots", "segments", "reps", "warmup", "thresh", "skip") for x in ("--" + k, str(getattr(a, k)))] + \
                  ["--time-thresh", str(a.time_thresh), "--center-time", str(a.center_time), "--frame-dist", str(a.frame_dist)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("SIDE_JSON ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a side that did not end clean
                print(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode or 1
            out[mode][side] = json.loads(line[0][len("SIDE_JSON "):])
            with open(a.out, "w") as f:                          # (kept after every side: a later one may run out of time)
                json.dump(out, f)
        same = out[mode]["this"]["digest_of_the_last_stage"] == out[mode]["parent"]["digest_of_the_last_stage"]
        out[mode]["same_pools_at_the_last_stage"] = same
        ok = ok and same
        for u, w in zip(out[mode]["this"]["steps"], out[mode]["parent"]["steps"]):
            u["parent_over_this"] = w["seconds_median"] / u["seconds_median"]
            print(f"{mode} step {u['step']}: {sum(u['submaps'])} submaps, {sum(u['frames'])} frames; this {1e3 * u['seconds_median']:.2f} ms "
                  f"({1e3 * u['seconds_min']:.2f} - {1e3 * u['seconds_max']:.2f}), {u['frame_bytes_uploaded'] / 1e6:.2f} MB up, {u['reselected']} of {u['total']} reselected; "
                  f"parent {1e3 * w['seconds_median']:.2f} ms ({1e3 * w['seconds_min']:.2f} - {1e3 * w['seconds_max']:.2f}), {w['frame_bytes_uploaded'] / 1e6:.2f} MB up; "
                  f"parent / this {u['parent_over_this']:.2f}")
        print(f"{mode}: same pools at the last stage:", same)
    with open(a.out, "w") as f:
        json.dump(out, f)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
