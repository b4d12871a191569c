"""Frame-descriptor submaps without a GPU: the NumPy restatement (tests/_frame_desc_oracle.py) against what the
reference's own submaps_from_roman_map and Submap.similarity gave (tests/golden/frame_desc_golden.npz), the seeded cases of
tests/test_gpu_frame_desc.py checked clean, and build_submap_pool(frames=...) + submap_align_pools over stand-in contexts against
to_submaps() + submap_align_grid on the same pools, for the three descriptor modes."""
import numpy as np
import pytest

import _frame_desc_oracle as fo
import _lc_tail
import _submaps_oracle as so
import test_gpu_frame_desc as tg
import test_grid_gate_cpu as tc
from roman_amd.align import SubmapAlignParams
from roman_amd.align import submap_align as sa
from roman_amd.align.submaps import FrameTable, MapTable, SubmapParams, build_submap_pool, submap_centers

SHARED, GOLDEN = fo.golden_cases()


class FrameSubmapContext(fo.FrameCallsMixin, so.OracleSubmapContext):
    """submaps_dev and frame_select_dev through the oracles."""


class FramePoolsContext(fo.FrameCallsMixin, tc.PoolsStubContext):
    """The batch call, the gate and the tail of tests/test_grid_gate_cpu.py plus stacked_sim_dev and grid_gate_sim_dev."""


def _golden_pool_inputs(case):
    cap = SHARED["kw"]["max_size"]
    n = len(case["src"])
    count = np.array([len(x) for x in case["src"]], dtype=np.int32)
    src = np.full((n, cap), -1, dtype=np.int32)
    for q, x in enumerate(case["src"]):
        src[q, :len(x)] = x
    return count, src


# ---------------------------------------------------------------------------------------------
# the oracle against the reference's own results
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_oracle_equals_the_reference(case):
    count, src = _golden_pool_inputs(case)
    pos = SHARED["trajectory"][:, :3, 3]
    mean = case["mode"] == 'mean_frame_descriptor'
    thin = case["frame_descriptor_dist"] if not mean else None
    assert not fo.borderline(count, src, SHARED["times"], SHARED["traj_times"], pos, thin)
    o = fo.frame_select_oracle(count, src, SHARED["times"], SHARED["traj_times"], pos, SHARED["frame_desc"], thin, want_mean=mean)
    assert len(o["sel"]) == len(case["sel"]) >= 10
    for got, want in zip(o["sel"], case["sel"]):
        assert np.array_equal(got, want)                                                           # selection: exact
    assert min(len(x) for x in case["sel"]) >= 1 and len({len(x) for x in case["sel"]}) > 1
    if mean:
        assert tg.close(o["mean"], case["mean"])
        ob = fo.frame_select_oracle(count, src, SHARED["times"], SHARED["traj_times"], pos, SHARED["frame_desc_b"], None, want_mean=True)
        assert tg.close(ob["mean"], case["mean_b"])
        import _grid_gate_oracle as go
        side = lambda m: dict(pos=np.zeros((len(m), 3)), pos_gt=None, T_w=np.tile(np.eye(4), (len(m), 1, 1)), time=np.zeros(len(m)), desc=m)
        sim = go.grid_gate_oracle(side(o["mean"]), side(ob["mean"]), radius=1.0)["sim"]
    else:
        assert not fo.borderline_sim(SHARED["frame_desc"], o["sel"], SHARED["frame_desc_b"], o["sel"])
        sim = fo.stacked_sim_oracle(SHARED["frame_desc"], o["sel"], SHARED["frame_desc_b"], o["sel"])
    assert tg.close(sim, case["sim"])
    assert case["sim"].max() - case["sim"].min() > 0.3                                             # the fixture's similarities are spread


def test_thinning_changes_the_selection_in_the_fixture():
    by = {c["name"]: c for c in GOLDEN}
    assert all(len(a) > len(b) >= 1 and set(b) <= set(a) and a[0] == b[0] for a, b in zip(by["stacked_all"]["sel"], by["stacked_10m"]["sel"]))


def test_borderline_detector_flags_what_it_should():
    c = tg.select_case()
    assert not fo.borderline(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], tg.THIN)
    o = fo.frame_select_oracle(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], None, tg.THIN)
    t2 = c["frame_times"].copy(); t2[20] = o["span"][3, 0] + 4e-10
    assert fo.borderline(c["count"], c["src"], c["seg_times"], t2, c["frame_pos"], None)
    assert fo.borderline(c["count"], c["src"], c["seg_times"], c["frame_times"], c["frame_pos"], float(o["steps"][5]) + 3e-10)
    desc0, desc1, sel0, sel1 = tg.stacked_case(19)
    sim = fo.stacked_sim_oracle(desc0, sel0, desc1, sel1)
    assert not fo.borderline_sim(desc0, sel0, desc1, sel1, 0.5)
    assert fo.borderline_sim(desc0, sel0, desc1, sel1, float(sim[0, 1]) - 4e-10)
    d2 = desc0.copy(); d2[5] = 0.0; d2[5, 0] = 1e-9 / np.linalg.norm(desc1[7])
    assert fo.borderline_sim(d2, sel0, desc1, sel1)
    with pytest.raises(AssertionError):
        fo.clean(fo.borderline_sim(d2, sel0, desc1, sel1), "planted")


def test_mask_round_trip():
    sel = [np.array([0, 63, 64, 69]), np.array([], dtype=np.int64), np.arange(70)]
    m = fo.pack_mask(sel, 70)
    assert m.shape == (3, 2) and m[0, 0] == (1 | (1 << 63)) and m[0, 1] == (1 | (1 << 5))
    from roman_amd.runtime import mask_indices
    for s in range(3):
        assert np.array_equal(fo.unpack_mask(m[s]), sel[s]) and np.array_equal(mask_indices(m[s]), sel[s])


# ---------------------------------------------------------------------------------------------
# every seeded case of the GPU tests is clean and hits the edges it is there for
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sorted_times,thin", tg.SELECT_CASES, ids=[c[0] for c in tg.SELECT_CASES])
def test_gpu_select_cases_are_clean(name, sorted_times, thin):
    c = tg.select_case(sorted_times)
    tg.check_select_case(c, thin)
    assert sorted_times == bool(np.all(np.diff(c["frame_times"]) > 0))


@pytest.mark.parametrize("d", [3, 19, 64])
def test_gpu_stacked_cases_are_clean(d):
    tg.check_stacked_case(d)
    _, _, sel0, sel1 = tg.stacked_case(d)
    assert len(set(sel0[0]) & set(sel0[2])) > 0 and len(set(sel1[0]) & set(sel1[1])) > 0      # the same frame sits in several submaps


def test_gpu_gate_case_is_clean():
    a, b, o = tg.gate_case()
    assert np.all(np.abs(o["sim"] - tg.GATE["desc_thresh"]) > 1e-9)


# ---------------------------------------------------------------------------------------------
# build_submap_pool(frames=...) on a stand-in against the reference's fixture
# ---------------------------------------------------------------------------------------------
def _registration():
    return SubmapAlignParams(method="roman", semantics_dim=16).get_object_registration()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_build_submap_pool_with_frames_equals_the_reference(case):
    reg = _registration()
    table = MapTable(SHARED["feats"], SHARED["times"], SHARED["ids"], 3, 16)
    params = SubmapParams(**SHARED["kw"], submap_descriptor=case["mode"], frame_descriptor_dist=case["frame_descriptor_dist"])
    centers = submap_centers(list(SHARED["trajectory"]), SHARED["traj_times"], params)
    frames = FrameTable.from_map(list(SHARED["trajectory"]), SHARED["traj_times"], list(SHARED["frame_desc"]))
    ctx = FrameSubmapContext()
    pool = build_submap_pool(reg, table, centers, params, ctx=ctx, device="cpu", frames=frames)
    assert ctx.calls == 1 and ctx.frame_selects == 1 and ctx.syncs == 1
    assert np.array_equal(pool.nonempty, case["sm_id"])
    fm = pool.frame_mask.numpy().view(np.uint64)
    for q, s in enumerate(pool.nonempty):
        assert np.array_equal(fo.unpack_mask(fm[s]), case["sel"][q]) and pool.frame_n[s] == len(case["sel"][q])
    class _Seg:
        pass
    subs = pool.to_submaps([_Seg() for _ in range(len(table))])
    for q, sm in enumerate(subs):
        if case["mode"] == 'mean_frame_descriptor':
            assert sm.descriptor.shape == (16,) and tg.close(sm.descriptor, case["mean"][q])
        else:
            assert np.array_equal(sm.descriptor, SHARED["frame_desc"][case["sel"][q]])


def test_build_submap_pool_refusals():
    reg = _registration()
    table = MapTable(SHARED["feats"], SHARED["times"], SHARED["ids"], 3, 16)
    traj, times = list(SHARED["trajectory"]), SHARED["traj_times"]
    for mode in ('mean_frame_descriptor', 'stacked_frame_descriptors'):
        params = SubmapParams(**SHARED["kw"], submap_descriptor=mode)
        with pytest.raises(ValueError, match="frames="):
            build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=FrameSubmapContext(), device="cpu")
    # a non-empty submap whose span holds no frame: the reference fails on it, and so does this
    params = SubmapParams(**SHARED["kw"], submap_descriptor='stacked_frame_descriptors')
    frames = FrameTable.from_map(traj, times + 1.0e6, list(SHARED["frame_desc"]))
    with pytest.raises(ValueError, match="submap 0 holds"):
        build_submap_pool(reg, table, submap_centers(traj, times, params), params, ctx=FrameSubmapContext(), device="cpu", frames=frames)
    with pytest.raises(ValueError, match="one entry per frame"):
        FrameTable.from_map(traj, times[:-1], list(SHARED["frame_desc"]))


# ---------------------------------------------------------------------------------------------
# submap_align_pools over stand-ins against submap_align_grid, the end-to-end case of the GPU test
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tg.E2E, ids=[c["name"] for c in tg.E2E])
def test_pools_path_equals_grid_path_on_a_stand_in(case):
    build, made = FrameSubmapContext(), []

    def make(pools):
        made.append(FramePoolsContext(int(pools[0].pool.shape[0] + pools[1].pool.shape[0]), 3))
        return made[0]
    got, want, pools = tg.run_e2e(case, make, "cpu", build_ctx=build, compute=_lc_tail.oracle_lc_compute)
    ctx = made[0]
    stacked = case["mode"] == 'stacked_frame_descriptors'
    assert build.frame_selects == 2 and ctx.gates == 1 and ctx.tails == 1 and getattr(ctx, "stacked_sims", 0) == (1 if stacked else 0)
    assert ctx.order[0] == ("stacked_sim" if stacked else "gate") and ctx.order[-1] == "tail" and "batch" in ctx.order
    tc.assert_same_results(got, want)
    tg.compare_e2e(case, got, want)
    # the threshold splits the pairs, and no decision is borderline (1e-9, as the oracles' detectors ask)
    sim = want.similarity_mat
    assert np.nanmin(np.abs(sim - case["thresh"])) > 1e-9
    for q in pools:
        thin = case["dist"] if stacked else None
        assert not fo.borderline(q.count, q.src, q.table.times, q.frames.times, q.frames.pos, thin)
    if stacked:
        sel = [[fo.unpack_mask(m) for m in q.frame_mask.numpy().view(np.uint64)[q.nonempty]] for q in pools]
        assert not fo.borderline_sim(pools[0].frames.desc, sel[0], pools[1].frames.desc, sel[1], case["thresh"])
        assert any(len(set(a) & set(b)) for a in sel[0] for b in sel[0] if a is not b)          # frames shared between submaps


def test_pools_path_refuses_pools_built_another_way():
    reg, pools, _ = tc._pools("roman", 'mean_semantic')
    base = dict(method="roman", semantics_dim=tc.D, submap_radius=15.0)
    for mode in ('mean_frame_descriptor', 'stacked_frame_descriptors'):
        with pytest.raises(ValueError, match="frames="):
            sa.submap_align_pools(SubmapAlignParams(**base, submap_descriptor=mode), pools, sa.SubmapAlignIO(), registration=reg)


def test_demo_parameters_run_through_the_pools_path():
    """The reference demo's submap_descriptor, frame_descriptor_dist and submap_descriptor_thresh (params/demo/submap_align.yaml)."""
    case = dict(name="demo", mode='stacked_frame_descriptors', dist=10.0, thresh=0.8)
    make = lambda pools: FramePoolsContext(int(pools[0].pool.shape[0] + pools[1].pool.shape[0]), 3)
    got, want, _ = tg.run_e2e(case, make, "cpu", build_ctx=FrameSubmapContext(), compute=_lc_tail.oracle_lc_compute)
    tc.assert_same_results(got, want)
