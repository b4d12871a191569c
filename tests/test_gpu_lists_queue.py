"""k_lists' pair sweep (kernels.hip.h): the set bits of the mask words go through a per-wave LDS queue and are placed 256 at a
time with every lane busy; a wave step with more pairs than the queue holds goes in 64 at a time.  The lists it builds against
the four-kernel path's (ROMAN_LISTS=0: the symmetric matrix, k_rowsort, k_upper) on live sets that stress the queue: the
largest the stream layout takes, a few rows holding most of the pairs, rows without a pair, dense rows, config-3 batches and
a list pool too small for the first attempt.  roman_get_upper_csr sorts its rows: the order of entries inside a row is free."""
import numpy as np
import pytest

from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import batch as rb

pytestmark = pytest.mark.gpu

STREAM_MAXL = 3072


def _both_paths(ctx, reg, pr, monkeypatch, A=None):
    """score + solve with ROMAN_LISTS=0 and =1 (each with k_count taking whole problems and row blocks): the same upper CSR,
    the same iterate bit for bit, the same nodes and pass counts.  Returns the CSR."""
    reg.set_context(ctx)
    P = reg._abi_params()
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    if A is None:
        A = reg._association_list(pr.map1, pr.map2)
    runs = []
    for lists, whole in (("0", "0"), ("1", "1"), ("1", "0")):
        monkeypatch.setenv("ROMAN_LISTS", lists)
        monkeypatch.setenv("ROMAN_COUNT_WHOLE", whole)
        ctx.score(P, D1, D2, A)
        csr = [x.copy() for x in ctx.upper_csr()]
        ctx.solve(None)
        nodes, u, score, st = ctx.solution()
        runs.append((csr, nodes.copy(), u.copy(), score, (st.n_live, st.nnz_upper, st.n_pass, st.outer_iters, st.inner_iters, st.ls_trials)))
    ref = runs[0]
    for got in runs[1:]:
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert got[3] == ref[3] and got[4] == ref[4]
    return ref[0], ref[4]


def test_live_set_at_the_stream_layouts_limit(ctx, monkeypatch):
    # every association live (a zero single score removes nothing): 48 x 64 = 3072 = STREAM_MAXL live rows, the most words per row
    reg = registration_for("roman", semantics_dim=32)
    reg._abi_params().single_mode = 3
    pr = synth.make_pair(48, 64, 32, 61)
    (rp, cc, vv, dd), stats = _both_paths(ctx, reg, pr, monkeypatch)
    assert stats[0] == STREAM_MAXL and stats[1] > 0


def _hub_pair(n_hub, n_shell, n_far, seed):
    """Both maps: n_hub objects within 1e-3 of the origin, n_shell on a sphere of radius 10 around it (the same in both maps),
    n_far far away (a kilometre out in map 1, five in map 2).  An association of two hub objects is consistent with every
    association of two shell objects (both distances are 10): the n_hub^2 hub rows hold most of the pairs; an association of a
    far object is consistent with nothing."""
    rng = np.random.default_rng(seed)
    hub = rng.uniform(-1e-3, 1e-3, (n_hub, 3))
    d = rng.standard_normal((n_shell, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = 10.0 * d
    far1 = 1000.0 + rng.uniform(-300.0, 300.0, (n_far, 3))
    far2 = -5000.0 + rng.uniform(-300.0, 300.0, (n_far, 3))
    n = n_hub + n_shell + n_far
    pr = synth.make_pair(n, n, 0, seed)
    for objs, far in ((pr.map1, far1), (pr.map2, far2)):
        for o, p in zip(objs, np.vstack([hub, shell, far])):
            o.centroid = p.reshape(3, 1).copy()
    return pr


@pytest.mark.parametrize("n_hub", [2, 4])
def test_a_few_rows_hold_most_pairs_and_some_rows_none(ctx, monkeypatch, n_hub):
    reg = registration_for("clipper", epsilon=0.005, sigma=0.004)
    pr = _hub_pair(n_hub, 48 - n_hub, 6, 70 + n_hub)
    (rp, cc, vv, dd), stats = _both_paths(ctx, reg, pr, monkeypatch)
    L = len(rp) - 1
    assert 0 < L <= STREAM_MAXL
    # full degrees from the upper CSR: the n_hub^2 hub rows hold over a third of the stored pairs, hundreds of rows hold none
    deg = np.diff(rp).astype(np.int64)
    np.add.at(deg, cc, 1)
    top = np.sort(deg)[::-1][:n_hub * n_hub]
    assert top.sum() > 0.35 * deg.sum() / 2 and top[0] > 0.6 * L
    assert (deg == 0).sum() > 0


def test_dense_rows_take_the_queue_sixty_four_at_a_time(ctx, monkeypatch):
    # a third of all pairs consistent: a wave step of four rows x sixteen words has far more bits than the queue holds
    reg = registration_for("clipper", epsilon=4.0, sigma=2.0)
    pr = synth.make_pair(52, 52, 0, 31)
    (rp, cc, vv, dd), stats = _both_paths(ctx, reg, pr, monkeypatch)
    L = len(rp) - 1
    assert L > 2000 and stats[1] > 0.25 * L * (L - 1) / 2


def _run(reg, batch, ctx, monkeypatch, lists):
    monkeypatch.setenv("ROMAN_LISTS", lists)
    return rb.run_batch(reg, batch, ctx=ctx)


def _same_results(a, b, B):
    assert np.array_equal(a.status, b.status)
    for i in range(B):
        assert np.array_equal(a.assoc[i], b.assoc[i]), i
    assert np.array_equal(a.T, b.T, equal_nan=True)
    for f in ("n_live", "nnz_upper", "n_pass", "outer_iters", "inner_iters", "ls_trials", "score"):
        assert np.array_equal(a.stats[f], b.stats[f]), f


def test_config3_batch_equals_the_four_kernel_path(ctx, monkeypatch):
    reg = registration_for("semanticgrav", semantics_dim=512); reg.set_context(ctx)
    pairs = [synth.make_pair(200, 200, 512, 5100 + k) for k in range(256)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    four = _run(reg, batch, ctx, monkeypatch, "0")
    lists = _run(reg, batch, ctx, monkeypatch, "1")
    _same_results(lists, four, len(batch))
    assert (four.status == _abi.ROMAN_ST_OK).all() and (four.stats["n_live"] > 1000).all()


def test_list_pool_overflow_is_retried_and_equals_a_sized_call(monkeypatch):
    # a fresh context whose first attempt gets a list pool of 5 000 entries: k_lists marks the problems that do not fit
    # (kind 2), the library issues them again with the pool the history asks for
    from roman_amd.runtime import Context
    reg = registration_for("semanticgrav", semantics_dim=64)
    pairs = [synth.make_pair(60 + (k % 5) * 20, 70, 64, 5400 + k) for k in range(48)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    out = {}
    for name, cap in (("sized", None), ("overflow", "5000")):
        if cap is None:
            monkeypatch.delenv("ROMAN_TEST_CAPLIST", raising=False)
        else:
            monkeypatch.setenv("ROMAN_TEST_CAPLIST", cap)
        c = Context(0)
        try:
            reg.set_context(c)
            out[name] = _run(reg, batch, c, monkeypatch, "1")
            if cap is not None:
                assert c.skipped() > 0, "the first attempt's list pool did not overflow"
        finally:
            c.close()
    _same_results(out["overflow"], out["sized"], len(batch))
    assert not (out["sized"].status & _abi.ROMAN_ST_WORKSPACE).any()


@pytest.mark.parametrize("window", ["0", "1000", "20000"], ids=["no_window", "window_496", "window_10000"])
def test_lds_window_of_any_size_builds_the_same_lists(ctx, monkeypatch, window):
    # ROMAN_LISTS_LDS: the window of list entries k_lists builds in LDS (bytes; default: all the LDS the kernel leaves).  None, one
    # that ends inside the first rows' lists and one that ends in the middle of the problem: the lists of the four-kernel path
    reg = registration_for("clipper", epsilon=0.005, sigma=0.004)
    pr = _hub_pair(3, 45, 6, 77)
    monkeypatch.setenv("ROMAN_LISTS_LDS", window)
    (rp, cc, vv, dd), stats = _both_paths(ctx, reg, pr, monkeypatch)
    assert stats[1] > 2 * 20000
