"""Self loop closures over device-resident pools on the device: one robot drives a loop twice (tests/_self_pools.py),
build_submap_pool once, then submap_align_pools(p, [pool, pool]) — the call that raised ValueError before roman_shared_reduce_dev —
against submap_align_grid on to_submaps() of the same pool.  torch holds the device memory, so the comparison runs in a process of
its own with torch imported first (as tests/test_gpu_submap_align_pools.py does), with that file's tolerances:

exact: association counts, robots_nearby_mat, every association array, the accepted pairs; 1e-12: poses, T_ij, edges, similarity;
1e-9: angle, distance and yaw matrices.

tests/_self_pools.conditions() asserts what keeps the comparison from passing vacuously (8-16 submaps, nothing left on the diagonal,
registered pairs that lost some / nothing, accepted closures between laps only, a pair the time gate stopped).  Pools with disjoint
ids and single_robot_lc=True make no roman_shared_reduce_dev call."""
import subprocess
import sys

import pytest


def run_all_on_the_device():
    import torch
    import numpy as np
    import _self_pools as sp
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    calls = []
    reduce_dev = ctx.shared_reduce_dev
    ctx.shared_reduce_dev = lambda *a, **kw: (calls.append(int(a[0])), reduce_dev(*a, **kw))[1]
    for case in sp.CASES:
        calls.clear()
        got, want, pool = sp.run_case(case, ctx, dev)              # (raised ValueError before the removal had a device-pointer form)
        seen = sp.conditions(case, want, pool)
        sp.compare(got, want)
        assert calls == [len(got.timing_list)], calls                # one call over every registered pair
        assert pool.ids_dev is not None and np.array_equal(pool.ids_dev.cpu().numpy(), pool.ids.reshape(-1))
        print(f"{case['name']}: {seen}")
    # two maps with their own ids under single_robot_lc: the path without the removal
    import test_gpu_submap_align_pools as tp
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    p = SubmapAlignParams(method="gravity", semantics_dim=tp.D, submap_radius=15.0, submap_center_dist=30.0, submap_max_size=40,
                          single_robot_lc=True, single_robot_lc_time_thresh=20.0)
    reg = p.get_object_registration(); reg.set_context(ctx)
    params = SubmapParams.from_submap_align_params(p)
    pools = []
    for r, (sg, traj, times) in enumerate(tp.make_maps(False)):
        for q in sg:
            q.id = int(q.id) + 100000 * r
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=ctx, device=dev))
    calls.clear()
    res = sa.submap_align_pools(p, pools, sa.SubmapAlignIO(lc_association_thresh=4), registration=reg)
    assert calls == [] and len(res.timing_list) > 0
    ctx.close()
    print("SELF_POOLS_OK")


@pytest.mark.gpu
def test_self_pools_equal_the_grid_path_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_self_pools as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SELF_POOLS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
