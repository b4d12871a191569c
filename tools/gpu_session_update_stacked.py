"""A growing session at the reference demo's descriptor settings ('stacked_frame_descriptors', frame_descriptor_dist 10.0,
submap_descriptor_thresh 0.8): what a step pays for its similarity + gate when the similarity follows the pair list
(roman_session_stacked_sim_list_dev) and when it is computed for whole blocks (the parent commit).

  python tools/gpu_session_update_stacked.py --parent-root /path/to/a/built/checkout/of/the/parent --out profiles/session_update_stacked/timing.json

Scale: tools/gpu_session_stacked.py's four robots with frame tables (10^4 segments, 2000 poses, 768-d frame descriptors, about 100
submaps each, the 10 blocks r <= s).  The pools are built once per process at their final size; a step's pools are their first
S_r - K + k submaps.  Per repetition a fresh state, the full first call (step 0), then K steps that append one submap per robot.
Per step: the device time of similarity + gate (two events on the context's stream: in front of the similarity call, behind
roman_session_gate_list_dev) and the wall time of the step.  `this`: this tree's package and library; `parent`: the package and
library under --parent-root (skipped without it).  `full_list`: on this tree, the list call at the FULL list against the
whole-block call over the final pools, events around each — the one point where the list call has no pair to leave out.
Each way in a process of its own under `timeout -k 10`, 3 warm-up repetitions, 10 timed, every sample kept; the next way starts
only after a clean end of the one before; the last step's results of `this` and `parent` are compared.  No ratio is promised."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT = 420            # seconds per way
SIM_CALLS = ("session_stacked_sim_dev", "session_stacked_sim_list_dev")


def prefix(pool, k):
    """The first k submaps of `pool` as a pool of its own (the frame table is the map's and stays whole)."""
    c = pool.centers
    cen = dataclasses.replace(c, **{f.name: getattr(c, f.name)[:k] for f in dataclasses.fields(c)})
    cut = lambda a, n: None if a is None else a[:n]
    return dataclasses.replace(pool, pool=pool.pool[:k * pool.cap], count=pool.count[:k], src=pool.src[:k], ids=pool.ids[:k], status=pool.status[:k],
                               desc=cut(pool.desc, k), centers=cen, desc_dev=cut(pool.desc_dev, k), ids_dev=cut(pool.ids_dev, k * pool.cap),
                               frame_mask=cut(pool.frame_mask, k), frame_n=cut(pool.frame_n, k))


def stats(x, unit):
    return {unit + "_median": float(np.median(x)), unit + "_min": float(np.min(x)), unit + "_max": float(np.max(x)), unit: [float(v) for v in x]}


def setup(a):
    import gpu_session_stacked as gst                        # (its own sys.path entry first; the package comes from --root, in front of it)
    sys.path.insert(0, a.root)
    return gst, gst.setup(a)


def run_way(a):
    """The growing session with this process's package: -> one row per step."""
    gst, (torch, dev, stream, ctx, p, io, reg, final, blocks) = setup(a)
    from roman_amd.align import submap_align as sa
    n = [len(q.count) for q in final]
    pools_at = [[prefix(q, m - a.steps + k) for q, m in zip(final, n)] for k in range(a.steps + 1)]
    ev, used = {}, []

    def before(name):                                        # an event in front of the similarity call ...
        f = getattr(ctx, name)

        def call(*args, **kw):
            ev["e0"] = torch.cuda.Event(enable_timing=True); ev["e0"].record(stream)
            used.append(name)
            return f(*args, **kw)
        setattr(ctx, name, call)
    for name in SIM_CALLS:
        if hasattr(ctx, name):
            before(name)
    gate = ctx.session_gate_list_dev

    def gate_then_event(*args, **kw):                        # ... and one behind the list gate
        r = gate(*args, **kw)
        ev["e1"] = torch.cuda.Event(enable_timing=True); ev["e1"].record(stream)
        return r
    ctx.session_gate_list_dev = gate_then_event
    rows = [dict(step=k, submaps=[int(len(q.nonempty)) for q in pools_at[k]]) for k in range(a.steps + 1)]
    wall, dev_ms = [[] for _ in rows], [[] for _ in rows]
    for rep in range(a.warmup + a.reps):
        state = sa.SessionAlignState()
        for k, pools in enumerate(pools_at):
            del used[:]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = sa.submap_align_session_update(state, p, pools, None, blocks, io, registration=reg)
            torch.cuda.synchronize(dev)
            if rep >= a.warmup:
                wall[k].append(time.perf_counter() - t0)
                dev_ms[k].append(ev["e0"].elapsed_time(ev["e1"]))
            rows[k].update(listed_pairs=int(state.listed), all_pairs=int(state.total), similarity_call=list(used),
                           registered=int(sum(len(r.timing_list) for r in res.values())), loop_closures=int(sum(len(r.lc_edges["pairs"]) for r in res.values())))
    for k, row in enumerate(rows):
        row.update(stats(wall[k], "seconds")); row.update(stats(dev_ms[k], "similarity_and_gate_ms"))
    np.savez(a.dump, **gst.summary(res, blocks))
    ctx.close()
    return rows


def run_full_list(a):
    """The list call over EVERY pair of the final pools against the whole-block call over the same tables, events around each."""
    gst, (torch, dev, stream, ctx, p, io, reg, pools, blocks) = setup(a)
    from roman_amd.runtime import session_tables
    keep = [q.nonempty for q in pools]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    counts = [len(k) for k in keep]
    sub_off, blk, pair_off, _ = session_tables(counts, [(r, s, r == s) for r, s in blocks])
    masks = [q.frame_mask[torch.from_numpy(k.astype(np.int64)).to(dev)].contiguous() for q, k in zip(pools, keep)]
    nf = [int(q.frame_desc_dev.shape[0]) for q in pools]
    frame_lo = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int32); frame_n = np.array(nf, dtype=np.int32)
    mask_off = np.concatenate([[0], np.cumsum([int(m.numel()) for m in masks])[:-1]]).astype(np.int64)
    host = (frame_lo, frame_n, mask_off, sub_off, blk, pair_off)
    dtab = [up(x) for x in host]
    fdesc, fmask = torch.cat([q.frame_desc_dev for q in pools]), torch.cat([m.reshape(-1) for m in masks])
    total = int(pair_off[-1])
    lst = np.array([(b, i, j) for b, (r, s) in enumerate(blocks) for i in range(counts[r]) for j in range(counts[s])], dtype=np.int32).reshape(-1, 3)
    dlist = up(lst)
    sim = {k: torch.full((total,), -5.5, dtype=torch.float64, device=dev) for k in ("whole_blocks", "full_list")}
    head = (gst.D, int(fdesc.shape[0]), fdesc.data_ptr(), fmask.data_ptr()) + host
    ptrs = [x.data_ptr() for x in dtab]
    calls = dict(whole_blocks=lambda: ctx.session_stacked_sim_dev(*head, *ptrs, sim["whole_blocks"].data_ptr()),
                 full_list=lambda: ctx.session_stacked_sim_list_dev(*head, lst, *ptrs, dlist.data_ptr(), sim["full_list"].data_ptr()))
    out = dict(pairs=total, frames=nf, d=gst.D)
    for name, fn in calls.items():
        ms = []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            fn()
            e1.record(stream)
            ctx.sync(); e1.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        out[name] = stats(ms, "ms")
    out["similarity_bits_equal"] = bool(sim["whole_blocks"].cpu().numpy().tobytes() == sim["full_list"].cpu().numpy().tobytes())
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--way", default=None, choices=["this", "parent", "full_list"], help="(internal) run one way in this process")
    ap.add_argument("--root", default=ROOT, help="(internal) the tree whose package and library the way imports")
    ap.add_argument("--parent-root", dest="parent_root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--steps", type=int, default=4, help="appending steps behind the full first call")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference demo's)")
    ap.add_argument("--frame-dist", dest="frame_dist", type=float, default=10.0, help="frame_descriptor_dist (the reference demo's)")
    ap.add_argument("--window", type=int, default=40, help="poses over which two frames' descriptors decorrelate")
    ap.add_argument("--skip", type=float, default=float("inf"))
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_update_stacked", "timing.json"))
    a = ap.parse_args()
    if a.way:
        print("WAY_JSON " + json.dumps(run_full_list(a) if a.way == "full_list" else run_way(a)))
        return 0
    out = dict(scale=dict(robots=a.robots, segments=a.segments, d=768, method="roman", submap_descriptor="stacked_frame_descriptors",
                          frame_descriptor_dist=a.frame_dist, thresh=a.thresh, steps=a.steps, reps=a.reps, warmup=a.warmup))
    ways = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent_root))] if a.parent_root else []) + [("full_list", ROOT)]
    dumps = {}
    with tempfile.TemporaryDirectory() as td:
        for way, root in ways:
            dumps[way] = os.path.join(td, way + ".npz")
            env = dict(os.environ, ROMAN_HIP_LIBRARY=os.path.join(root, "roman_amd", "csrc", "libroman_hip.so"))
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--way", way, "--root", root, "--dump", dumps[way]] + \
                  [x for k in ("steps", "robots", "segments", "reps", "warmup", "thresh", "skip", "window") for x in ("--" + k, str(getattr(a, k)))] + \
                  ["--time-thresh", str(a.time_thresh), "--frame-dist", str(a.frame_dist)]
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("WAY_JSON ")]
            if r.returncode != 0 or not line:                # nothing more is started on the device after a way that did not end clean
                print(f"way {way} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return r.returncode or 1
            out[way] = json.loads(line[0][len("WAY_JSON "):])
            print(way, "done", flush=True)
        if "parent" in dumps:
            za, zb = np.load(dumps["this"]), np.load(dumps["parent"])
            out["same_results_at_the_last_step"] = bool(sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    for k, u in enumerate(out["this"]):
        w = out["parent"][k] if "parent" in out else None
        print(f"step {u['step']}: listed {u['listed_pairs']} of {u['all_pairs']} pairs through {u['similarity_call']}: similarity + gate "
              f"{u['similarity_and_gate_ms_median']:.3f} ms, step {1e3 * u['seconds_median']:.1f} ms" +
              (f"; parent {w['similarity_and_gate_ms_median']:.3f} ms, step {1e3 * w['seconds_median']:.1f} ms" if w else ""))
    f = out["full_list"]
    print(f"full list of {f['pairs']} pairs: list call {f['full_list']['ms_median']:.3f} ms, whole-block call {f['whole_blocks']['ms_median']:.3f} ms, "
          f"bits equal: {f['similarity_bits_equal']}")
    print("same results at the last step:", out.get("same_results_at_the_last_step"))
    return 0 if out.get("same_results_at_the_last_step", True) and f["similarity_bits_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
