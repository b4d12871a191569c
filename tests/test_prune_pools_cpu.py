"""method='clipper+prune' on the device-resident path without a GPU: submap_align_pools and submap_align_session
with the device-prefilter plugin (DistRegWithPruning.on_device()) over the stand-in contexts of the neighbouring CPU tests — the
gate through tests/_grid_gate_oracle.py, the batch through the CPU oracle (ROMAN_INV_EUCLIDEAN_PRUNED: the prefilter as a 0/1
single score), the tail through tests/_lc_tail.py — against submap_align_grid with the `oracle_lc_compute` double; the refusals
for pools the kernel would misread; on_device() itself; and the batched path of submap_align_grid for such a plugin."""
import copy
import dataclasses

import numpy as np
import pytest

import _lc_tail
import _self_pools as sp
import _session as ss
import _submaps_oracle as so
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.dist_reg_with_pruning import DistRegWithPruning
from roman_amd.align.object_registration import ObjectRegistration
from test_grid_gate_cpu import assert_same_results

D = 16
BASE = dict(method="clipper+prune", semantics_dim=D, submap_radius=15.0, cosine_min=0.5, epsilon_shape=0.03)
VIEWS = [dict(keep=1.0, first_pose=0, max_size=12), dict(keep=0.85, first_pose=3, max_size=10)]


class RecordingContext(ss.SessionStubContext):
    """The session stand-in, remembering the parameter block of every batch call and the tilt threshold of every tail."""

    def __init__(self):
        super().__init__()
        self.blocks, self.tilts = [], []

    def align_batch_dev(self, P, *a, **kw):
        self.blocks.append(_abi.RomanParams.from_buffer_copy(P))
        return super().align_batch_dev(P, *a, **kw)

    def lc_tail_dev(self, lp, *a, **kw):
        self.tilts.append(float(lp.tilt_thresh))
        return super().lc_tail_dev(lp, *a, **kw)


def device_plugin(**kw):
    """The documented way: the factory's plugin (NumPy prefilter), then on_device()."""
    host = SubmapAlignParams(**{**BASE, **kw}).get_object_registration()
    assert isinstance(host, DistRegWithPruning) and not host.prune_on_device
    return host.on_device(D)


def build_pools(reg, n_robots, descriptor='mean_semantic'):
    """`n_robots` views of one place (tests/_session.robot_view: own segments, ids and centres), each in a pool packed by `reg`."""
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    base = synth.make_map(90, D, seed=31, n_poses=24, dt=8.0)
    pools, segs = [], []
    for r in range(n_robots):
        v = VIEWS[r]
        params = SubmapParams(max_size=v["max_size"], radius=15.0, time_threshold=np.inf, pruning_method='distance', submap_descriptor=descriptor)
        sg, traj, times = ss.robot_view(*base, r, keep=v["keep"], first_pose=v["first_pose"])
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=so.OracleSubmapContext(), device="cpu"))
        segs.append(sg)
    return pools, segs


SELF = dict(method="clipper+prune", descriptor=None, thresh=0.0)      # a case of tests/_self_pools.py: two laps of one map, loops close between the laps


def self_params(**kw):
    p, io = sp.params_of(SELF)
    return dataclasses.replace(p, cosine_min=BASE["cosine_min"], epsilon_shape=BASE["epsilon_shape"], **kw), io


def check_blocks(ctx, reg):
    assert ctx.blocks and ctx.tilts
    for P in ctx.blocks:
        assert P.invariant == _abi.ROMAN_INV_EUCLIDEAN_PRUNED and P.cos_feature_dim == D and P.ratio_feature_dim == 4
        assert P.cosine_min == reg.cos_min and all(P.ratio_epsilon[f] == reg.shape_epsilon for f in range(4))
    assert all(t == reg.roll_pitch_thresh for t in ctx.tilts)           # the plugin's own roll / pitch check rides in the tail


@pytest.mark.parametrize("kind", ["cross-mean-semantic", "self-shared-ids"])
def test_pools_reach_the_gate_and_the_batch_with_the_device_prefilter(kind):
    reg = device_plugin()
    if kind.startswith("cross"):
        pl, sg = build_pools(reg, 2)
        p, io = SubmapAlignParams(**BASE, submap_descriptor='mean_semantic', submap_descriptor_thresh=0.8), sa.SubmapAlignIO(lc_association_thresh=4)
    else:                                                    # one pool against itself: the rows pass through the gather region at full width
        pool, segs = sp.build_pool(SELF, reg, so.OracleSubmapContext(), "cpu")
        pl, sg = [pool, pool], [segs, segs]
        p, io = self_params()
    ctx = RecordingContext(); reg.set_context(ctx)
    ctx.n_objects = int(sum(q.pool.shape[0] for q in pl)) if kind.startswith("cross") else 0
    assert int(pl[0].pool.shape[1]) == 3 + 4 + D and pl[0].table.desc_dim == D
    got = sa.submap_align_pools(p, pl, io, registration=reg)
    assert ctx.gates == 1 and ctx.tails == 1 and ctx.order[0] == "gate" and ctx.order[-1] == "tail" and "batch" in ctx.order
    assert ("reduce" in ctx.order) == (kind == "self-shared-ids")
    check_blocks(ctx, reg)
    want = sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pl, sg)], io, registration=reg, compute=_lc_tail.oracle_lc_compute)
    assert_same_results(got, want)
    assert (want.clipper_num_associations >= 4).sum() >= 2, "no pair of the grid aligned: the comparison would show nothing"
    # ... and the prefilter had something to remove in an aligned pair (the reference's NumPy prefilter on the same submaps)
    host = SubmapAlignParams(**BASE).get_object_registration()
    subs = [q.to_submaps(s) for q, s in zip(pl, sg)]
    i, j = np.argwhere(want.clipper_num_associations >= 4)[0]
    kept = len(host._associations_to_score(subs[0][i].segments, subs[1][j].segments))
    assert 0 < kept < len(subs[0][i]) * len(subs[1][j])


def test_session_reaches_the_gate_and_the_batch_with_the_device_prefilter():
    """Robot 0 drives two laps (its self block closes loops between them), robot 1 the first lap of the same place."""
    from roman_amd.align.submaps import MapTable, SubmapParams, build_submap_pool, submap_centers
    reg = device_plugin()
    p, io = self_params(submap_descriptor='mean_semantic', submap_descriptor_thresh=0.65)
    params = SubmapParams.from_submap_align_params(p)
    pools = []
    for r, last in ((0, None), (1, sp.N_POSES)):
        sg, traj, times = ss.robot_view(*sp.two_lap_map(), r, keep=1.0 - 0.15 * r, last_pose=last)
        pools.append(build_submap_pool(reg, MapTable.from_segments(reg, sg), submap_centers(traj, times, params), params, ctx=so.OracleSubmapContext(), device="cpu"))
    blocks = [(0, 0), (0, 1)]
    ctx = RecordingContext(); reg.set_context(ctx)
    want = {}
    for r, s in blocks:
        q = copy.copy(p); q.single_robot_lc = (r == s)
        ctx.n_objects = int(pools[r].pool.shape[0] + pools[s].pool.shape[0])
        want[(r, s)] = sa.submap_align_pools(q, [pools[r], pools[s]], io, registration=reg)
    ctx2 = RecordingContext(); reg.set_context(ctx2)
    ctx2.n_objects = int(sum(q.pool.shape[0] for q in pools))
    got = sa.submap_align_session(p, pools, blocks, io, registration=reg)
    assert list(got) == blocks
    assert ctx2.session_gates == 1 and ctx2.gates == 0 and ctx2.tails == 1 and ctx2.order.count("reduce") == 1 and "batch" in ctx2.order
    check_blocks(ctx2, reg)
    aligned = 0
    for key in blocks:
        ss.compare(got[key], want[key])
        aligned += int((want[key].clipper_num_associations >= 4).sum())
    assert aligned >= 2, "hardly a pair aligned: the comparison would show nothing"
    assert all((want[k].clipper_num_associations >= 4).any() for k in ((0, 0), (0, 1))), "a self block and a cross block must both align a pair"


def _no_context(reg):
    reg._context = lambda: (_ for _ in ()).throw(AssertionError("a context was made"))
    return reg


def test_pools_the_kernel_would_misread_are_refused_before_a_context_is_made():
    import torch
    reg = _no_context(device_plugin())
    pools, _ = build_pools(reg, 2)
    roman = SubmapAlignParams(method="roman", semantics_dim=D).get_object_registration()
    roman_pools, _ = build_pools(roman, 2)
    assert int(roman_pools[0].pool.shape[1]) == int(pools[0].pool.shape[1]), "method='roman' rows have the same width here: only the table tells them apart"
    wide = dataclasses.replace(pools[1], pool=torch.cat([pools[1].pool, pools[1].pool[:, :1]], dim=1))
    other_d = dataclasses.replace(pools[1], table=dataclasses.replace(pools[1].table, desc_dim=8))
    unset = _no_context(device_plugin()); unset.semantics_dim = None
    p, io = SubmapAlignParams(**BASE), sa.SubmapAlignIO()
    cases = [(reg, [pools[0], wide], "dim + 4 + semantics_dim"), (reg, [wide, wide], "dim + 4 + semantics_dim"), (reg, [pools[0], other_d], "desc_dim"),
             (unset, pools, "semantics_dim"), (reg, roman_pools, "another registration")]
    for r, pl, what in cases:
        with pytest.raises(ValueError, match="to_submaps") as e:
            sa.submap_align_pools(p, pl, io, registration=r)
        assert what in str(e.value) and "submap_align_grid" in str(e.value), (what, str(e.value))
        with pytest.raises(ValueError, match="submap_align_pools") as e:
            sa.submap_align_session(p, pl, None, io, registration=r)
        assert what in str(e.value), (what, str(e.value))
    # the factory's plugin keeps its host prefilter, and so does a third-party plugin with a scorer of its own — also one
    # derived from DistRegWithPruning with the switch set
    class Own(ObjectRegistration):
        def _associations_to_score(self, map1, map2):
            return None

    class OwnPrune(DistRegWithPruning):
        def _associations_to_score(self, map1, map2):
            return None
    host = _no_context(SubmapAlignParams(**BASE).get_object_registration())
    derived = _no_context(OwnPrune(0.4, 0.6, prune_on_device=True, semantics_dim=D))
    assert sa._has_host_prefilter(host) and sa._has_host_prefilter(Own()) and sa._has_host_prefilter(derived)
    assert not sa._has_host_prefilter(reg) and not sa._has_host_prefilter(roman)
    for r in (host, derived):
        with pytest.raises(ValueError, match="prefilters association lists on the host"):
            sa.submap_align_pools(p, pools, io, registration=r)
        with pytest.raises(ValueError, match="prefilters association lists on the host"):
            sa.submap_align_session(p, pools, None, io, registration=r)


def test_on_device_copies_the_thresholds_and_leaves_the_original():
    host = DistRegWithPruning(0.3, 0.5, mindist=0.1, shape_epsilon=0.07, cos_min=0.66, dim=3, use_gravity=True, roll_pitch_thresh=0.05)
    before = dict(vars(host))
    assert host._ctx is None and host.on_device(D)._ctx is None             # no context set: none made
    ctx = object(); host.set_context(ctx); before["_ctx"] = ctx
    dev = host.on_device(D)
    assert dev is not host and type(dev) is DistRegWithPruning and dev.prune_on_device and dev.semantics_dim == D and dev._ctx is ctx
    for k in ("sigma", "epsilon", "mindist", "shape_epsilon", "cos_min", "dim", "use_gravity", "roll_pitch_thresh"):
        assert getattr(dev, k) == getattr(host, k), k
    assert vars(host) == before and not host.prune_on_device and host.semantics_dim is None
    assert host._abi_params().invariant == _abi.ROMAN_INV_EUCLIDEAN
    P = dev._abi_params()
    assert P.invariant == _abi.ROMAN_INV_EUCLIDEAN_PRUNED and P.cos_feature_dim == D and P.ratio_feature_dim == 4 and P.cosine_min == 0.66
    assert dev.on_device().semantics_dim == D and dev.on_device(8).semantics_dim == 8 and dev.semantics_dim == D
    # the factory's output stays the reference's
    f = SubmapAlignParams(**BASE).get_object_registration()
    assert not f.prune_on_device and f._abi_params().invariant == _abi.ROMAN_INV_EUCLIDEAN


@pytest.mark.parametrize("single_robot_lc", [False, True])
def test_submap_align_grid_makes_one_batched_call_without_association_lists(single_robot_lc):
    reg = device_plugin()
    pools, segs = build_pools(reg, 2, None)
    p = SubmapAlignParams(**BASE, single_robot_lc=single_robot_lc, single_robot_lc_time_thresh=40.0)
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    pl, sg = ([pools[0], pools[0]], [segs[0], segs[0]]) if single_robot_lc else (pools, segs)
    subs = [q.to_submaps(s) for q, s in zip(pl, sg)]
    seen, tilts = [], []

    def compute(registration, batch, lc):
        seen.append(batch); tilts.append(lc.tilt_thresh)
        return _lc_tail.oracle_lc_compute(registration, batch, lc)
    res = sa.submap_align_grid(p, subs, io, registration=reg, compute=compute)
    assert len(seen) == 1 and seen[0].assoc is None and seen[0].assoc_off is None
    assert int(seen[0].feats.shape[1]) == 3 + 4 + D and len(seen[0]) == len(res.timing_list) >= 4
    assert tilts == [reg.roll_pitch_thresh]
    # the host-prefilter plugin on the same submaps still hands over its lists
    host = SubmapAlignParams(**BASE).get_object_registration()
    seen.clear()
    sa.submap_align_grid(p, [q.to_submaps(s) for q, s in zip(pl, sg)], io, registration=host, compute=compute)
    assert len(seen) == 1 and seen[0].assoc is not None and int(seen[0].feats.shape[1]) == 3
