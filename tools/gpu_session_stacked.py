"""A session of R robots at the reference demo's descriptor settings — submap_descriptor 'stacked_frame_descriptors',
frame_descriptor_dist 10.0, submap_descriptor_thresh 0.8 — to loop closures: ONE submap_align_session call against
the loop of submap_align_pools over the same robot pairs (the only way to run that session before the session call took the mode),
on the same device-resident pools, and the device time of the similarity + gate alone (roman_session_stacked_sim_dev and
roman_session_gate_sim_dev between two events, against roman_stacked_sim_dev + roman_grid_gate_sim_dev per block).

  python tools/gpu_session_stacked.py --out profiles/session_stacked/timing.json

Scale: tools/gpu_session.py's four maps of one place (100, 95, 90, 85 % of 10^4 segments, about 100 submap centres each), every
pose a frame with a 768-d descriptor that decorrelates over 40 poses of the drive (each robot's copy with noise of its own; the robots open the drive
40 poses apart, so their frame tables differ in length): the 10 blocks r <= s, the 4 self blocks with the shared-segment removal.
The pools are built once per process, outside the timed region.  Each path runs in a process of its own under `timeout -k 10`: 3
warm-up calls, then the median of 10, and the library calls and synchronisations of one timed repetition counted by entry point;
the parent starts the next step only after a clean end, compares the two paths' results and writes the JSON.  No ratio is promised:
the numbers are what they are."""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 768
DS = 16                                                  # segment descriptors (not read by the stacked mode)
LIMITS = dict(session=420, loop=420, gate=300)            # seconds per step


def setup(a):
    import torch
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import FrameTable, MapTable, SubmapParams, build_submap_pool, submap_centers
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    p = SubmapAlignParams(method="roman", semantics_dim=DS, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40,
                          submap_descriptor='stacked_frame_descriptors', frame_descriptor_dist=a.frame_dist, submap_descriptor_thresh=a.thresh,
                          single_robot_lc_time_thresh=a.time_thresh)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=a.skip)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    segs, traj, times = synth.make_map(a.segments, DS, seed=8100, n_poses=2000, loop_radius=125.0, laps=1.3, dt=1.0)
    # a frame's descriptor: the sum of the `window` independent vectors that start at its pose — two frames k poses apart have the
    # cosine 1 - k / window, so the descriptor gate passes submaps that saw the same stretch of the drive and stops the others
    run = np.cumsum(np.random.default_rng(8150).normal(0.0, 1.0, (len(traj) + a.window, D)), axis=0)
    drift = run[a.window:] - run[:-a.window]
    pools = []
    for r in range(a.robots):
        # the same place mapped by every robot (cross pairs have true matches), each with its own view of it: 100, 95, 90, ... % of
        # the segments, every centre a few cm off, ids of its own, the drive opened 40 poses later per robot
        rng = np.random.default_rng(8200 + r)
        pick = np.sort(rng.permutation(len(segs))[:int(round((1.0 - 0.05 * r) * len(segs)))])
        mine = []
        for k in pick.tolist():
            q = copy.copy(segs[k])
            q.id = int(segs[k].id) + 10 ** 6 * r
            q.centroid = np.asarray(segs[k].centroid, dtype=np.float64) + rng.normal(0.0, 0.03, size=np.shape(segs[k].centroid))
            mine.append(q)
        desc = drift[40 * r:] + 0.02 * rng.normal(0.0, 1.0, (len(traj) - 40 * r, D))
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, mine), submap_centers(traj[40 * r:], times[40 * r:], params), params, ctx=ctx, device=dev,
                                       frames=FrameTable.from_map(traj[40 * r:], times[40 * r:], list(desc))))
    blocks = [(r, s) for r in range(a.robots) for s in range(r, a.robots)]
    return torch, dev, stream, ctx, p, io, reg, pools, blocks


def summary(results, blocks):
    out = {}
    for b, key in enumerate(blocks):
        res = results[key]
        out[f"n{b}"] = np.nan_to_num(res.clipper_num_associations, nan=-1.0); out[f"nearby{b}"] = np.nan_to_num(res.robots_nearby_mat, nan=-1.0)
        out[f"pairs{b}"] = np.asarray(res.lc_edges["pairs"]); out[f"t{b}"] = np.asarray(res.lc_edges["t"]); out[f"q{b}"] = np.asarray(res.lc_edges["q"])
        out[f"That{b}"] = np.nan_to_num(res.T_ij_hat_mat, nan=0.0); out[f"sim{b}"] = np.nan_to_num(res.similarity_mat, nan=-2.0, neginf=-3.0)
    return out


def count_calls(ctx, calls):
    """Every public entry of the context counts itself into `calls` (library calls and synchronisations by name)."""
    for name in dir(ctx):
        f = getattr(ctx, name)
        if name.startswith("_") or not callable(f) or not (name.endswith("_dev") or name in ("sync", "join")):
            continue

        def counted(*args, _f=f, _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*args, **kw)
        setattr(ctx, name, counted)


def step_path(a, which):
    from roman_amd.align import submap_align as sa
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a)
    secs, calls = [], {}
    count_calls(ctx, calls)
    for rep in range(a.warmup + a.reps):
        calls.clear()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if which == "session":
            res = sa.submap_align_session(p, pools, blocks, io, registration=reg)
        else:
            res = {}
            for r, s in blocks:
                q = copy.copy(p); q.single_robot_lc = (r == s)
                res[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
        torch.cuda.synchronize(dev)
        if rep >= a.warmup:
            secs.append(time.perf_counter() - t0)
    out = dict(seconds_median=float(np.median(secs)), seconds_min=float(np.min(secs)), seconds_max=float(np.max(secs)), seconds=[float(x) for x in secs], blocks=len(blocks),
               submaps=[int(len(q.nonempty)) for q in pools], frames=[int(q.frame_desc_dev.shape[0]) for q in pools],
               frames_per_submap_mean=[float(np.mean(q.frame_n[q.nonempty])) for q in pools], calls_of_one_repetition=dict(sorted(calls.items())), registered=int(sum(len(r.timing_list) for r in res.values())),
               loop_closures=int(sum(len(r.lc_edges["pairs"]) for r in res.values())))
    np.savez(a.dump, **summary(res, blocks))
    ctx.close()
    return out


def step_gate(a):
    """The similarity and the gate alone, between two events: the session's two calls, and the per-block pairs of calls."""
    from roman_amd.runtime import grid_gate_params, session_tables
    torch, dev, stream, ctx, p, io, reg, pools, blocks = setup(a)
    keep = [q.nonempty for q in pools]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    counts = [len(k) for k in keep]
    tabs = session_tables(counts, [(r, s, r == s) for r, s in blocks])
    dtab = [up(x) for x in tabs]
    pose = [q.centers.pose_flu[k] for q, k in zip(pools, keep)]
    pos, T_w, tm = [up(x[:, :3, 3]) for x in pose], [up(x.reshape(-1, 16)) for x in pose], [up(q.centers.time[k]) for q, k in zip(pools, keep)]
    masks = [q.frame_mask[torch.from_numpy(k.astype(np.int64)).to(dev)].contiguous() for q, k in zip(pools, keep)]
    fd = [q.frame_desc_dev for q in pools]
    nf = [int(x.shape[0]) for x in fd]
    frame_lo = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int32); frame_n = np.array(nf, dtype=np.int32)
    mask_off = np.concatenate([[0], np.cumsum([int(m.numel()) for m in masks])[:-1]]).astype(np.int64)
    ftab = [up(frame_lo), up(frame_n), up(mask_off)]
    fdesc, fmask = torch.cat(fd), torch.cat([m.reshape(-1) for m in masks])
    cat = lambda xs: torch.cat(xs).contiguous()
    pos_all, T_all, tm_all = cat(pos), cat(T_w), cat(tm)
    B, nb = int(tabs[2][-1]), len(blocks)
    f64, i32 = torch.float64, torch.int32
    o = [torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=f64, device=dev),
         torch.empty(16 * B, dtype=f64, device=dev), torch.empty(2 * B, dtype=i32, device=dev), torch.empty(16 * B, dtype=f64, device=dev),
         torch.empty(B, dtype=i32, device=dev), torch.zeros(nb + 1, dtype=i32, device=dev)]
    n_todo = torch.zeros(1, dtype=i32, device=dev)
    gp = grid_gate_params(15.0, a.skip, 0, a.thresh, False, a.time_thresh)

    def session():
        ctx.session_stacked_sim_dev(D, int(fdesc.shape[0]), fdesc.data_ptr(), fmask.data_ptr(), frame_lo, frame_n, mask_off, tabs[0], tabs[1], tabs[2],
                                    *[x.data_ptr() for x in ftab], dtab[0].data_ptr(), dtab[1].data_ptr(), dtab[2].data_ptr(), o[3].data_ptr())
        ctx.session_gate_dev(gp, *tabs, *[x.data_ptr() for x in dtab], pos_all.data_ptr(), T_all.data_ptr(), *[x.data_ptr() for x in o],
                             time_ptr=tm_all.data_ptr(), sim_in_ptr=o[3].data_ptr())

    def per_block():
        for b, (r, s) in enumerate(blocks):
            lo = int(tabs[2][b])
            at = lambda t, w, size: t.data_ptr() + lo * w * size
            ctx.stacked_sim_dev(D, nf[r], fd[r].data_ptr(), counts[r], masks[r].data_ptr(), nf[s], fd[s].data_ptr(), counts[s], masks[s].data_ptr(), at(o[3], 1, 8))
            gq = grid_gate_params(15.0, a.skip, 0, a.thresh, r == s, a.time_thresh)
            ctx.grid_gate_sim_dev(gq, counts[r], counts[s], pos[r].data_ptr(), T_w[r].data_ptr(), pos[s].data_ptr(), T_w[s].data_ptr(), at(o[0], 1, 8), at(o[1], 1, 4),
                                  at(o[2], 1, 8), at(o[3], 1, 8), at(o[4], 16, 8), at(o[5], 2, 4), at(o[6], 16, 8), at(o[7], 1, 4), n_todo.data_ptr(),
                                  time0_ptr=tm[r].data_ptr(), time1_ptr=tm[s].data_ptr())
    out = dict(blocks=nb, pairs=B, d=D, frames=nf)
    sims = {}
    for name, fn in (("session_calls", session), ("per_block_calls", per_block)):
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
        out[name + "_ms_median"] = float(np.median(ms)); out[name + "_ms_min"] = float(np.min(ms))
        sims[name] = o[3].cpu().numpy().copy()
    out["n_todo_session"] = int(o[8].cpu().numpy()[-1])
    out["similarity_bits_equal"] = bool(sims["session_calls"].tobytes() == sims["per_block_calls"].tobytes())
    ctx.close()
    return out


def same_results(fa, fb, nb):
    A, B = np.load(fa), np.load(fb)
    exact = all(np.array_equal(A[f"{k}{b}"], B[f"{k}{b}"]) for b in range(nb) for k in ("n", "nearby", "pairs", "sim"))
    tol = all(A[f"{k}{b}"].shape == B[f"{k}{b}"].shape and np.allclose(A[f"{k}{b}"], B[f"{k}{b}"], rtol=0, atol=1e-12) for b in range(nb) for k in ("t", "q", "That"))
    return bool(exact and tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=["session", "loop", "gate"], help="(internal) run one step in this process")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.8, help="submap_descriptor_thresh (the reference demo's)")
    ap.add_argument("--frame-dist", dest="frame_dist", type=float, default=10.0, help="frame_descriptor_dist (the reference demo's)")
    ap.add_argument("--window", type=int, default=40, help="poses over which two frames' descriptors decorrelate")
    ap.add_argument("--skip", type=float, default=float("inf"), help="skip_distance")
    ap.add_argument("--time-thresh", dest="time_thresh", type=float, default=50.0, help="single_robot_lc_time_thresh of the self blocks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_stacked", "timing.json"))
    a = ap.parse_args()
    if a.step:
        res = step_gate(a) if a.step == "gate" else step_path(a, a.step)
        print("STEP_RESULT " + json.dumps(res))
        return 0
    nb = a.robots * (a.robots + 1) // 2
    out = dict(scale=dict(robots=a.robots, blocks=nb, segments=a.segments, d=D, method="roman", submap_descriptor="stacked_frame_descriptors",
                          frame_descriptor_dist=a.frame_dist, thresh=a.thresh, reps=a.reps, warmup=a.warmup))
    names = dict(session="session_call", loop="loop_of_submap_align_pools", gate="similarity_and_gate_alone")
    with tempfile.TemporaryDirectory() as td:
        for step in ("session", "loop", "gate"):
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--dump", os.path.join(td, step + ".npz"),
                   "--robots", str(a.robots), "--segments", str(a.segments), "--reps", str(a.reps), "--warmup", str(a.warmup), "--thresh", str(a.thresh),
                   "--skip", str(a.skip), "--time-thresh", str(a.time_thresh), "--frame-dist", str(a.frame_dist), "--window", str(a.window)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")]
            if r.returncode != 0 or not line:                    # nothing more is started on the device after a step that did not end cleanly
                print(f"step {step} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                return 1
            out[names[step]] = json.loads(line[0][len("STEP_RESULT "):])
            print(step, line[0], flush=True)
        out["same_results"] = same_results(os.path.join(td, "session.npz"), os.path.join(td, "loop.npz"), nb)
    out["loop_over_session"] = out["loop_of_submap_align_pools"]["seconds_median"] / out["session_call"]["seconds_median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if out["same_results"] else 2


if __name__ == "__main__":
    sys.exit(main())
