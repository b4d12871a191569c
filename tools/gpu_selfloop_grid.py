"""Self loop closures through submap_align_grid(): the shared-segment removal on the device (every submap packed and uploaded
once, roman_align_lc_batch_ids) against the per-pair removal on the host (two reduced lists packed per pair, roman_align_lc_batch
over the 2 B pool) on the same synthetic grid, phase by phase.

  python tools/gpu_selfloop_grid.py --grid 16 --out profiles/selfloop/selfloop_grid_demo_16.json

Demo scale: one robot, submaps of 20-40 objects with 768-d descriptors, method 'roman', `single_robot_lc=True`; both sides of the
grid are that robot's submaps, consecutive submaps share a third of their segments (overlapping id ranges) and every submap shares
all of them with itself.  The two forms run alternately in one process, `--reps` times each after one untimed warm-up each;
medians are reported.  Phases: pass 1 (everything before the device call, packing included), the device call, pass 2 / record
unpacking, loop_closure_edges; besides: calls into registration.pack, bytes handed to the device call (feature pool + ids), and
the share of problems that lost a segment."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roman_amd import synth                                   # noqa: E402
from roman_amd.align import SubmapAlignParams, batch as rb    # noqa: E402
from roman_amd.align import submap_align as sa                # noqa: E402


def make_self_grid(S, d=768, seed=0):
    rng = np.random.default_rng(seed)
    objs, poses = synth.make_submap_grid(S, n=40, d=d, seed0=5000, overlap=0.6)
    objs = [[o[q] for q in sorted(rng.choice(40, size=int(rng.integers(20, 41)), replace=False))] for o in objs]
    start = 0
    for segs in objs:                                           # consecutive id ranges overlap by a third of a submap
        for q, s in enumerate(segs):
            s.id = start + q
        start += len(segs) - len(segs) // 3
    robot = [sa.Submap(id=k, time=20.0 * k, segments=objs[k],
                       pose_flu=poses[k] @ synth.yaw_transform(0.0, [0, 0, 0], roll=rng.normal(0, 0.02), pitch=rng.normal(0, 0.02))) for k in range(S)]
    return [robot, copy.deepcopy(robot)]


def timed(params, io, reg, submaps, per_pair):
    """One run on a deep copy of the submaps -> dict of phase seconds and counters.  per_pair: inject run_lc_batch as `compute`
    (the removal per pair on the host); otherwise the default compute, whose device call is timed where the module makes it."""
    subs = copy.deepcopy(submaps)
    inner, packs = {}, []

    def around(fn):
        def call(registration, batch, lc):
            t0 = time.perf_counter()
            out = fn(registration, batch, lc)
            inner["t0"], inner["t1"] = t0, time.perf_counter()
            inner["bytes"] = int(batch.feats.nbytes + (0 if batch.ids is None else batch.ids.nbytes))
            inner["problems"] = len(batch)
            if out.n1_kept is not None:
                inner["affected"] = int(np.count_nonzero((out.n1_kept != batch.n1) | (out.n2_kept != batch.n2)))
            else:                                               # the host removed already: affected = shorter than its submap
                i, j = batch.pair_index[:, 0], batch.pair_index[:, 1]
                l0 = np.array([len(s) for s in subs[0]]); l1 = np.array([len(s) for s in subs[1]])
                inner["affected"] = int(np.count_nonzero((batch.n1 != l0[i]) | (batch.n2 != l1[j])))
            return out
        return call
    orig_pack, orig_entry = reg.pack, sa.run_lc_batch_ids
    reg.pack = lambda m: (packs.append(len(m)), orig_pack(m))[1]
    sa.run_lc_batch_ids = around(orig_entry)
    try:
        t_start = time.perf_counter()
        res = sa.submap_align_grid(params, subs, io, registration=reg, compute=around(rb.run_lc_batch) if per_pair else None)
        t_end = time.perf_counter()
    finally:
        reg.pack, sa.run_lc_batch_ids = orig_pack, orig_entry
    edges = sa.loop_closure_edges(res, subs)
    t_edges = time.perf_counter()
    return dict(pass1=inner["t0"] - t_start, device_call=inner["t1"] - inner["t0"], pass2=t_end - inner["t1"],
                loop_closure_edges=t_edges - t_end, total=t_edges - t_start, n_edges=len(edges), pack_calls=len(packs),
                bytes_uploaded=inner["bytes"], problems=inner["problems"], affected_share=inner["affected"] / max(inner["problems"], 1),
                n_assoc_sum=int(np.nansum(res.clipper_num_associations)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    submaps = make_self_grid(a.grid)
    params = SubmapAlignParams(method="roman", semantics_dim=768, submap_radius=1e3, single_robot_lc=True, single_robot_lc_time_thresh=50.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    reg = params.get_object_registration()
    legs = {"ids_on_device": False, "per_pair_on_host": True}
    runs = {k: [] for k in legs}
    for rep in range(a.reps + 1):                               # alternating; repetition 0 warms both up and is dropped
        for name, per_pair in legs.items():
            t = timed(params, io, reg, submaps, per_pair)
            if rep:
                runs[name].append(t)
    out = dict(scale="demo", grid=a.grid, pairs=a.grid * a.grid, reps=a.reps, method="roman", d=768, single_robot_lc=True)
    for name in legs:
        out[name] = {k: float(np.median([r[k] for r in runs[name]])) for k in ("pass1", "device_call", "pass2", "loop_closure_edges", "total")}
        for k in ("n_edges", "pack_calls", "bytes_uploaded", "problems", "affected_share", "n_assoc_sum"):
            out[name][k] = runs[name][0][k]
    same = all(out["ids_on_device"][k] == out["per_pair_on_host"][k] for k in ("n_edges", "problems", "affected_share", "n_assoc_sum"))
    out["same_edges_and_association_counts"] = bool(same)
    out["speedup_total"] = out["per_pair_on_host"]["total"] / out["ids_on_device"]["total"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
