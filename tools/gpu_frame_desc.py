#!/usr/bin/env python3
"""Pass 1 of a two-map session with stacked frame descriptors at the reference demo's scale (about 60 submaps a side, about 3000
frames a map, 768-d descriptors), frame_descriptor_dist 10.0 and None:

  (a) the host way: the frame list of every submap built on the host as extract_submap_descriptors does [REF roman/map/map.py:210-242],
      stacked_similarity (Context.cosine_matrix over the STACKED lists + np.maximum.reduceat), the NumPy gate of submap_align_grid;
  (b) frame_select_dev x 2 + stacked_sim_dev + grid_gate_sim_dev on tensors that are already on the device.

Results are checked equal first (selections and flags exact, similarities 1e-12); then each way is run `--warmup` times untimed and
`--reps` times timed, wall clock around a synchronised call; medians, minima, maxima and the spread (max - min) / median go into
the JSON file with the distinct-pair and duplicated-pair counts.  Usage: python tools/gpu_frame_desc.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_side(rng, S, Nf, d, spacing, width):
    """Nf frames `spacing` metres and 0.5 s apart along a gently curving path; S submaps whose two segments span `width` frames
    around centres Nf / S frames apart (a frame belongs to about width * S / Nf submaps)."""
    t = 0.5 * np.arange(Nf) + 0.25
    ang = np.linspace(0.0, 1.5 * np.pi, Nf)
    R = Nf * spacing / (1.5 * np.pi)
    pos = np.stack([R * np.cos(ang), R * np.sin(ang), 0.2 * np.sin(5 * ang)], axis=1)
    x = rng.normal(0.0, 1.0, d) + 0.5
    desc = np.zeros((Nf, d))
    for f in range(Nf):
        x = x + 0.05 * rng.normal(0.0, 1.0, d)
        desc[f] = x
    centres = (np.arange(S) + 0.5) * Nf / S
    lo = np.clip(centres - width / 2, 0, Nf - 1); hi = np.clip(centres + width / 2, 0, Nf - 1)
    seg_times = np.stack([np.stack([0.5 * np.floor(lo), 0.5 * np.floor(lo) + 1.0], axis=1), np.stack([0.5 * np.floor(hi) - 1.0, 0.5 * np.floor(hi) + 0.5], axis=1)],
                         axis=1).reshape(2 * S, 2)
    count = np.full(S, 2, np.int32); src = np.arange(2 * S, dtype=np.int32).reshape(S, 2)
    ci = np.clip(centres.astype(int), 0, Nf - 1)
    T_w = np.tile(np.eye(4), (S, 1, 1)); T_w[:, :3, 3] = pos[ci]
    for s in range(S):
        c, sn = np.cos(ang[ci[s]]), np.sin(ang[ci[s]])
        T_w[s, :2, :2] = [[c, -sn], [sn, c]]
    return dict(times=t, pos=pos, desc=np.ascontiguousarray(desc), seg_times=seg_times, count=count, src=src, sm_pos=pos[ci].copy(), T_w=T_w,
                sm_time=t[ci].copy())


def host_lists(side, thin):
    """extract_submap_descriptors on the host -> list of (k, d) stacks, list of index arrays"""
    out, sel = [], []
    for s in range(len(side["count"])):
        rows = side["src"][s, :side["count"][s]]
        lo, hi = side["seg_times"][rows, 0].min(), side["seg_times"][rows, 1].max()
        idx = np.nonzero((side["times"] >= lo) & (side["times"] <= hi))[0]
        if thin is not None:
            keep, last = [], None
            for f in idx:
                if last is None or np.linalg.norm(side["pos"][f] - last) >= thin:
                    keep.append(f); last = side["pos"][f]
            idx = np.array(keep, dtype=np.int64)
        out.append(side["desc"][idx]); sel.append(idx)
    return out, sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--submaps", type=int, default=60)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_desc", "timing.json"))
    a = ap.parse_args()
    import torch
    from roman_amd import _abi
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.runtime import Context, frame_select_params, grid_gate_params, mask_indices
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(7)
    S, Nf, d = a.submaps, a.frames, a.d
    sides = [make_side(rng, S, Nf, d, 0.5, 3.0 * Nf / S) for _ in range(2)]
    sides[1]["desc"] = np.ascontiguousarray(sides[0]["desc"] + 0.3 * rng.normal(0.0, 1.0, (Nf, d)))
    thresh, radius = 0.9, 15.0
    p = SubmapAlignParams(method="roman", submap_radius=radius, submap_descriptor='stacked_frame_descriptors', submap_descriptor_thresh=thresh)
    io = sa.SubmapAlignIO()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    D = [{k: up(v) for k, v in s.items()} for s in sides]
    W = (Nf + 63) // 64
    masks = [torch.zeros((S, W), dtype=torch.int64, device=dev) for _ in range(2)]
    nsel = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
    span = [torch.zeros((S, 2), dtype=torch.float64, device=dev) for _ in range(2)]
    g = sa._gate_buffers(torch, dev, S, S)
    gp = grid_gate_params(radius, io.skip_distance, 0, thresh)
    stream.synchronize()
    result = dict(scale=dict(submaps=S, frames=Nf, d=d, thresh=thresh, reps=a.reps, warmup=a.warmup), settings={})
    for label, thin in (("frame_descriptor_dist_10", 10.0), ("frame_descriptor_dist_none", None)):
        fp = frame_select_params(thin, False)

        def host_way():
            lists = [host_lists(s, thin) for s in sides]
            sim = sa.stacked_similarity(ctx, lists[0][0], lists[1][0])
            dl = sides[0]["sm_pos"][:, None, :] - sides[1]["sm_pos"][None, :, :]
            dist = np.sqrt((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2])
            skip, gated = sa._gates(dist, sim, p, io)
            return lists, sim, skip, gated

        def device_way():
            for r in range(2):
                ctx.frame_select_dev(fp, S, 2, D[r]["count"].data_ptr(), D[r]["src"].data_ptr(), 2 * S, D[r]["seg_times"].data_ptr(), Nf,
                                     D[r]["times"].data_ptr(), masks[r].data_ptr(), nsel[r].data_ptr(), span[r].data_ptr(), frame_pos_ptr=D[r]["pos"].data_ptr())
            ctx.stacked_sim_dev(d, Nf, D[0]["desc"].data_ptr(), S, masks[0].data_ptr(), Nf, D[1]["desc"].data_ptr(), S, masks[1].data_ptr(), g["sim"].data_ptr())
            ctx.grid_gate_sim_dev(gp, S, S, D[0]["sm_pos"].data_ptr(), D[0]["T_w"].data_ptr(), D[1]["sm_pos"].data_ptr(), D[1]["T_w"].data_ptr(),
                                  *[t.data_ptr() for t in g.values()])
            ctx.sync()

        # results equal before anything is timed
        lists, sim_h, skip, gated = host_way()
        device_way()
        for r in range(2):
            m = masks[r].cpu().numpy().view(np.uint64)
            for s in range(S):
                assert np.array_equal(mask_indices(m[s]), lists[r][1][s]), (label, r, s)
        sim_d = g["sim"].cpu().numpy(); flags = g["flags"].cpu().numpy()
        assert np.all(np.abs(sim_d - sim_h) <= 1e-12 * np.maximum(1.0, np.abs(sim_h))), float(np.abs(sim_d - sim_h).max())
        clear = np.abs(sim_h - thresh) > 1e-9                   # (a similarity within rounding of the threshold may fall either way)
        assert np.array_equal(((flags & _abi.ROMAN_GRID_GATED) != 0)[clear], gated[clear]) and np.array_equal((flags & _abi.ROMAN_GRID_SKIP) != 0, skip)
        n0, n1 = [sum(len(x) for x in lists[r][1]) for r in range(2)]
        u0, u1 = [len(set(np.concatenate(lists[r][1]).tolist())) for r in range(2)]
        entry = dict(frames_per_submap_mean=[n0 / S, n1 / S], duplicated_pairs=int(n0 * n1), distinct_selected_pairs=int(u0 * u1),
                     pairs_contracted_on_device=int(Nf * Nf), gated=int(gated.sum()), todo=int((~gated & ~skip).sum()), same_results=True)
        for name, fn in (("host_way", host_way), ("device_way", device_way)):
            for _ in range(a.warmup):
                fn()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            ts = np.array(ts) * 1e3
            entry[name] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()), spread=float((ts.max() - ts.min()) / np.median(ts)))
        # the device way's kernels between events: selection, similarity, gate
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ks = []
        for _ in range(a.reps):
            ev[0].record(stream)
            ctx.stacked_sim_dev(d, Nf, D[0]["desc"].data_ptr(), S, masks[0].data_ptr(), Nf, D[1]["desc"].data_ptr(), S, masks[1].data_ptr(), g["sim"].data_ptr())
            ev[1].record(stream); ev[1].synchronize()
            ks.append(ev[0].elapsed_time(ev[1]))
        entry["stacked_sim_dev_ms_median"] = float(np.median(ks))
        result["settings"][label] = entry
        print(label, json.dumps(entry))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("FRAME_DESC_TIMING_OK")


if __name__ == "__main__":
    main()
