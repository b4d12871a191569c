"""grow_session_pools in the frame-descriptor modes on the device: three robots (tests/_session_grow_frames.py: one
without submaps, one whose 63 frames become 64 and 65, one whose frames are its poses), at most 6 submaps and 70 frames each, d = 8,
three steps, both modes.  After every step the grown pools equal build_session_pools over the same inputs byte for byte — frame masks,
counts, means and the frame table included —, and with 'stacked_frame_descriptors' submap_align_session_update over the grown pools
equals submap_align_session over fresh ones.  torch holds the device memory, so this runs in a process of its own with torch imported
first."""
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = [('mean_frame_descriptor', None), ('stacked_frame_descriptors', None), ('stacked_frame_descriptors', 4.0)]


def run_end_to_end():
    import torch
    import _session_grow_frames as gf
    import _session_submaps as sx
    import _session_update as su
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    from roman_amd.align.submaps import SubmapParams, build_session_pools, grow_session_pools
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    D = gf.sg.D
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    for mode, dist in MODES:
        p = SubmapAlignParams(method="roman", semantics_dim=D, submap_radius=15.0, submap_descriptor=mode, frame_descriptor_dist=dist,
                              submap_descriptor_thresh=0.55, single_robot_lc=True, single_robot_lc_time_thresh=40.0)
        reg = p.get_object_registration(); reg.set_context(ctx)
        params = SubmapParams(max_size=40, radius=15.0, distance=40.0, time_threshold=40.0, pruning_method='distance', submap_descriptor=mode,
                              frame_descriptor_dist=dist)
        session = gf.FrameSession(reg, params)
        io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=45.0)
        state, align_state, before = None, sa.SessionAlignState(), None
        kept = listed = total = 0
        for k in range(session.STEPS):
            tables, centers, frames = session.stage(k)
            assert max(len(c) for c in centers) <= 6 and max(len(f) for f in frames) <= 70 and frames[1].desc.shape[1] == 8
            pools, touched, state = grow_session_pools(state, reg, tables, centers, params, ctx=ctx, device=dev, frames=frames)
            want = build_session_pools(reg, tables, centers, params, ctx=ctx, device=dev, frames=frames)
            for got, w in zip(pools, want):
                sx.same_pool(got, w)
                gf.same_frames(got, w)
            assert state.frames_uploaded == sum(len(f) for f in frames) - (0 if before is None else sum(len(q.frames) for q in before))
            one = sa._one_storage(torch, [q.frame_desc_dev for q in pools[1:]])
            assert one is not None and one.data_ptr() == pools[1].frame_desc_dev.data_ptr()
            if k:
                expect = gf.frame_differs(before, want)
                for r in range(3):
                    assert np.array_equal(touched[r], expect[r]), (mode, k, r, touched[r], expect[r])
                kept += int(sum((~t).sum() for t in touched))
            listed += state.frames_listed; total += state.total
            if mode == 'stacked_frame_descriptors':
                got_lc = sa.submap_align_session_update(align_state, p, pools, touched, None, io, registration=reg)
                want_lc = sa.submap_align_session(p, want, None, io, registration=reg)
                assert list(got_lc) == list(want_lc) == blocks
                for key in blocks:
                    su.equal(got_lc[key], want_lc[key])
            before = want
        print(f"{mode} dist={dist}: {listed} of {total} slots reselected, {kept} old submaps left untouched")
    ctx.close()
    print("SESSION_GROW_FRAMES_OK")


def test_grown_frame_pools_equal_fresh_ones_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_session_grow_frames as t; t.run_end_to_end()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_GROW_FRAMES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
