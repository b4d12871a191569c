"""submap_align_session_update with 'stacked_frame_descriptors' on the device: the three small maps of
tests/test_gpu_submap_align_session_stacked.py with frame tables, a full first call on the pools cut back by three submaps per
robot, then three appending steps — after every call EQUAL to submap_align_session over the same pools, every block bit for bit,
similarity_mat included.  A counting proxy around the context shows which similarity call a step makes: the whole-block call on
the first, ONE roman_session_stacked_sim_list_dev and no whole-block call afterwards.  torch holds the device memory, so the
comparison runs in a process of its own with torch imported first (as tests/test_gpu_submap_align_session.py does)."""
import collections
import subprocess
import sys

import pytest

D = 16
STEPS = 4
WATCHED = ("session_stacked_sim_dev", "session_stacked_sim_list_dev", "session_gate_list_dev", "session_gate_dev")


class Counting:
    """Forwards everything to the context; counts the calls of WATCHED."""

    def __init__(self, ctx):
        self._ctx, self.calls = ctx, collections.Counter()

    def __getattr__(self, name):
        attr = getattr(self._ctx, name)
        if name not in WATCHED:
            return attr

        def counted(*args, **kw):
            self.calls[name] += 1
            return attr(*args, **kw)
        return counted


def run_case(ctx, device):
    import _session_update as su
    import test_gpu_submap_align_session_stacked as ts
    from roman_amd.align import SubmapAlignParams
    from roman_amd.align import submap_align as sa
    build = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); build.set_context(ctx)
    p, final = ts.make_pools(build, ctx, device)
    io = sa.SubmapAlignIO(lc_association_thresh=4, skip_distance=40.0)
    n = [len(q.count) for q in final]
    assert min(n) >= STEPS + 1, n
    blocks = [(r, s) for r in range(3) for s in range(r, 3)]
    state = sa.SessionAlignState()
    proxy = Counting(ctx)
    reg = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); reg.set_context(proxy)
    plain = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration(); plain.set_context(ctx)
    listed, decided = [], 0
    for step in range(STEPS):
        pools = final if step == STEPS - 1 else [su.pool_prefix(q, m - (STEPS - 1) + step) for q, m in zip(final, n)]
        proxy.calls.clear()
        got = sa.submap_align_session_update(state, p, pools, None, None, io, registration=reg)
        calls = dict(proxy.calls)
        want = sa.submap_align_session(p, pools, None, io, registration=plain)
        assert list(got) == list(want) == blocks
        for key in blocks:
            su.equal(got[key], want[key])                    # (exact, similarity_mat included: sim_atol 0)
        decided += int(gated_and_todo(want, ts.THRESH))
        listed.append((state.listed, state.total))
        assert (step == 0) == (state.listed == state.total), (step, listed)
        assert calls.get("session_gate_list_dev") == 1 and "session_gate_dev" not in calls, (step, calls)
        if step == 0:
            assert calls.get("session_stacked_sim_dev") == 1 and "session_stacked_sim_list_dev" not in calls, (step, calls)
        else:
            assert calls.get("session_stacked_sim_list_dev") == 1 and "session_stacked_sim_dev" not in calls, (step, calls)
    registered = sum(len(w.timing_list) for w in want.values()); accepted = sum(len(w.lc_edges["pairs"]) for w in want.values())
    assert decided >= 1, "no block holds a GATED and a TODO pair: the similarity decides nothing"
    assert registered >= 6 and accepted >= 1, "hardly a pair aligned: the comparison would show nothing"
    print(f"stacked update: listed / all pairs per step {listed}, {registered} pairs registered at the end, {accepted} accepted, submaps {n}")


def gated_and_todo(want, thresh):
    """A block that holds a pair the descriptor gate stopped AND a pair it let through (tests/test_session_stacked_cpu.gated_and_todo)."""
    import numpy as np
    with np.errstate(invalid="ignore"):
        return any((r.similarity_mat < thresh).any() and (r.similarity_mat >= thresh).any() for r in want.values() if r.similarity_mat is not None)


def run_all_on_the_device():
    import torch
    from roman_amd.runtime import Context
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev); torch.cuda.set_stream(stream)
    ctx = Context(0, stream=stream.cuda_stream)
    run_case(ctx, dev)
    ctx.close()
    print("SESSION_UPDATE_STACKED_OK")


@pytest.mark.gpu
def test_update_over_the_pair_list_equals_the_full_session_call_on_the_device():
    from conftest import ROOT
    code = (f"import torch, sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {ROOT + '/tests'!r}); "
            "import test_gpu_submap_align_session_update_stacked as t; t.run_all_on_the_device()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SESSION_UPDATE_STACKED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
