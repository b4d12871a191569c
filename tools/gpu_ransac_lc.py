#!/usr/bin/env python3
"""RANSAC loop closures over device-resident pools.  Not a test and not bench.py.

    python tools/gpu_ransac_lc.py [--parent-lib PATH/libroman_hip.so] [--reps 10]

The driver starts every GPU step as a child process under its own `timeout -k 10` and stops at the first non-zero status:
  e2e      the demo-scale scenario of tools/gpu_pools_grid.py (two maps of the same place cut into submaps of up to 40 objects, pools built for
           RomanRegistration with 768-d descriptors, mean_semantic gate at 0.8), ransac_iter 10^4:
           submap_align_pools(method='ransac') over the resident pools against the only way there was before —
           SubmapPool.to_submaps() + the pair-loop form submap_align() with a RansacReg — on the same pools; the read-back of a
           whole problems x kmax association block is timed on its own.
  packed   does the row stride cost the packed call anything?  Event time of roman_ransac_batch_dev on the 4096 pairs of
           tools/gpu_ransac.py at ransac_iter 10^4 through plain ctypes, so that ANY build of the library can be timed: this
           tree's and, with --parent-lib, the parent commit's (built from `git archive` of it), in interleaved child processes —
           parent, this, parent, this ... — each the median of --reps calls after warm-up.  The parent is measured twice per
           round, which gives the run-to-run spread the new median is held against.
-> profiles/ransac_lc/timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ransac_lc")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step_packed(a):
    """One library (a.lib), plain ctypes: roman_ctx_create, roman_ransac_batch_dev, roman_ctx_sync -> one JSON line."""
    import numpy as np
    import torch
    import gpu_ransac
    from roman_amd import _abi
    reg, bt = gpu_ransac.grid(4096)
    reg.max_iteration = 10 ** 4
    P = reg._ransac_params()
    lib = C.CDLL(a.lib)
    h = C.c_void_p()
    stream = torch.cuda.Stream()
    lib.roman_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.roman_ransac_batch_dev.argtypes = [C.c_void_p, C.POINTER(_abi.RomanRansacParams), C.c_int32] + [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 3
    lib.roman_ctx_destroy.argtypes = [C.c_void_p]
    assert lib.roman_ctx_create(C.byref(h), 0, C.c_void_p(stream.cuda_stream)) == 0
    B, kmax = len(bt), 64
    pts = torch.from_numpy(bt.feats).cuda()
    a_out = torch.zeros((B, kmax, 2), dtype=torch.int32, device="cuda")
    rec = torch.zeros(B * _abi.RANSAC_RECORD_NBYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.ctypes.data)
    off1, n1, off2, n2 = (np.ascontiguousarray(x) for x in (bt.off1.astype(np.int64), bt.n1.astype(np.int32), bt.off2.astype(np.int64), bt.n2.astype(np.int32)))

    def call():
        rc = lib.roman_ransac_batch_dev(h, C.byref(P), B, C.c_void_p(pts.data_ptr()), vp(off1), vp(n1), vp(off2), vp(n2), kmax,
                                        C.c_void_p(a_out.data_ptr()), C.c_void_p(rec.data_ptr()), None)
        assert rc == 0, rc
    ms = []
    with torch.cuda.stream(stream):
        for _ in range(3):
            call()
        stream.synchronize()
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    digest = int(np.frombuffer(rec.cpu().numpy().tobytes(), dtype=np.uint8).astype(np.uint64).sum())
    lib.roman_ctx_destroy(h)
    print(json.dumps(dict(lib=a.lib, median_ms=statistics.median(ms), ms=ms, pairs=B, record_bytes_sum=digest)), flush=True)


def step_e2e(a):
    import numpy as np
    import gpu_pools_grid as pg
    from roman_amd.align import RansacReg, SubmapAlignParams
    from roman_amd.align import submap_align as sa
    ns = argparse.Namespace(thresh=0.8, skip=float("inf"), segments=10000)
    torch, dev, stream, ctx, p, io, reg, params, maps = pg.setup(ns)
    pools = pg.build_pools(ctx, dev, reg, params, maps)
    pr = SubmapAlignParams(method="ransac", ransac_iter=10 ** 4, semantics_dim=pg.D, submap_radius=15.0, submap_center_dist=10.0, submap_max_size=40,
                           submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8)
    rr = RansacReg(max_iteration=10 ** 4); rr.set_context(ctx)
    t_pools, t_loop = [], []
    for rep in range(1 + a.e2e_reps):
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        got = sa.submap_align_pools(pr, pools, io, registration=rr)
        t1 = time.perf_counter()
        subs = [q.to_submaps(m[0]) for q, m in zip(pools, maps)]
        t2 = time.perf_counter()
        want = sa.submap_align(pr, subs, io, registration=rr)
        t3 = time.perf_counter()
        if rep:
            t_pools.append(t1 - t0); t_loop.append(dict(to_submaps=t2 - t1, submap_align=t3 - t2, total=t3 - t1))
    B = len(got.timing_list)
    same = bool(np.array_equal(got.clipper_num_associations, want.clipper_num_associations, equal_nan=True))
    kmax = int(max(q.count.max() for q in pools)) ** 2
    block = torch.zeros((B, kmax, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev); t0 = time.perf_counter(); block.cpu(); t_block = time.perf_counter() - t0
    med = lambda xs: float(statistics.median(xs))
    out = dict(submaps=[int(len(q.nonempty)) for q in pools], row_width=int(pools[0].pool.shape[1]), registered=B, ransac_iter=10 ** 4,
               loop_closures=int(len(got.lc_edges["pairs"])), association_counts_equal=same, timed_runs=a.e2e_reps,
               pools_path_s=med(t_pools), pair_loop_s={k: med([x[k] for x in t_loop]) for k in t_loop[0]},
               kmax=kmax, association_block_bytes=int(B) * kmax * 8, association_block_readback_s=t_block,
               note="the pools path reads back only the columns of the block that hold rows (the largest inlier count), not the block")
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["packed", "e2e"], default=None)
    ap.add_argument("--lib", default=os.path.join(ROOT, "roman_amd", "csrc", "libroman_hip.so"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--e2e-reps", type=int, default=3)
    a = ap.parse_args()
    if a.step == "packed":
        return step_packed(a)
    if a.step == "e2e":
        return step_e2e(a)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--e2e-reps", str(a.e2e_reps)]

    def child(name, limit, extra):
        print(f"[gpu_ransac_lc] step {name}", flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + me + extra, cwd=ROOT, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"[gpu_ransac_lc] step {name} ended with status {r.returncode}: stopping", flush=True)
            sys.exit(r.returncode)
        out = json.loads(r.stdout.strip().splitlines()[-1])
        out.pop("lib", None)                                      # (which build it was is the key it is filed under)
        return out
    rec = dict(packed=dict(this=[], parent=[]))
    for _ in range(a.rounds):                                       # parent, this, parent: interleaved, the parent twice per round
        for who, lib in (("parent", a.parent_lib), ("this", a.lib), ("parent", a.parent_lib)):
            if lib:
                rec["packed"][who].append(child(f"packed-{who}", 180, ["--step", "packed", "--lib", lib]))
    pk = rec["packed"]
    if pk["parent"]:
        pm = [x["median_ms"] for x in pk["parent"]]; tm = [x["median_ms"] for x in pk["this"]]
        pk["summary"] = dict(parent_medians_ms=pm, this_medians_ms=tm, parent_median_ms=statistics.median(pm), this_median_ms=statistics.median(tm),
                             parent_spread_ms=[min(pm), max(pm)], within_parent_spread=bool(min(pm) <= statistics.median(tm) <= max(pm)),
                             same_records=len({x["record_bytes_sum"] for x in pk["parent"] + pk["this"]}) == 1)
    rec["e2e"] = child("e2e", 900, ["--step", "e2e"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec.get("packed", {}).get("summary", {})), json.dumps(rec["e2e"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
