"""The shared-segment removal of self loop closures without a GPU: the NumPy model of the mark step against the reference's
wording (sets over `seg.id`), the two entry points at the C-ABI boundary, and submap_align_grid's default compute on a stub
runtime — every submap packed once, one batched call, the results of submap_align()."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

import _shared_ids as si
import test_submap_align as tsa
from conftest import ROOT
from roman_amd import _abi
from roman_amd.align import submap_align as sa
from test_submap_align_grid_cpu import assert_same_state, submap_state

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_shared_ids_dev", "roman_align_lc_batch_ids")


def check_model(ids, off1, n1, off2, n2):
    keep, kept = si.mark(ids, off1, n1, off2, n2)
    assert keep.shape == (int(n1.sum() + n2.sum()),) and keep.dtype == np.int32 and kept.shape == (len(n1), 2)
    for b, (k1, k2) in enumerate(si.kept_lists(keep, kept, n1, n2)):
        w1, w2 = si.reference_wording(ids[off1[b]:off1[b] + n1[b]].tolist(), ids[off2[b]:off2[b] + n2[b]].tolist())
        assert k1.tolist() == w1 and k2.tolist() == w2, b
    return keep, kept


def test_model_matches_the_reference_wording_on_the_edge_cases():
    ids, off1, n1, off2, n2, names = si.edge_batch()
    keep, kept = check_model(ids, off1, n1, off2, n2)
    by = dict(zip(names, kept.tolist()))
    assert by["1 x 1 equal"] == [0, 0] and by["1 x 1 unequal"] == [1, 1] and by["n1 = 0"] == [0, 3] and by["n2 = 0"] == [3, 0]
    assert by["all shared"] == [0, 0] and by["none shared"] == [70, 130] and by["the same submap on both sides"] == [0, 0]
    assert by["equal low words, different high words"] == [4, 4] and by["equal low words, one really equal"] == [1, 1]
    assert by["an id three times in one map, once in the other"] == [3, 2]          # all three repetitions go
    assert by["an id three times in one map, absent from the other"] == [5, 2]      # ... or all three stay
    assert by["negative ids"] == [2, 2] and by["last id of a 1030 map only"] == [1029, 2]
    assert by["shares its slice (1)"] == [40, 70] and by["shares its slice (2)"] == [60, 10]


def test_model_matches_the_reference_wording_on_random_cases():
    rng = np.random.default_rng(11)
    for trial in range(40):
        S = int(rng.integers(1, 6))
        lens = rng.integers(0, 50, S)
        span = int(rng.choice([3, 40, 10 ** 6]))             # few distinct ids (repetitions inside a map) ... hardly any collisions
        ids = rng.integers(-span, span, int(lens.sum())).astype(np.int64) * int(rng.choice([1, 1 << 33]))
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        B = int(rng.integers(1, 9))
        a, c = rng.integers(0, S, B), rng.integers(0, S, B)
        check_model(ids, offs[a], lens[a].astype(np.int32), offs[c], lens[c].astype(np.int32))
    ids, off1, n1, off2, n2 = si.small_batch()
    check_model(ids, off1, n1, off2, n2)


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and fn.argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    for s in ENTRY_POINTS:
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
    src = open(HEADER).read()
    # roman_align_lc_batch's 31 arguments plus ids, n1_kept, n2_kept, keep
    assert len(lib.roman_align_lc_batch_ids.argtypes) == len(lib.roman_align_lc_batch.argtypes) + 4 == 35
    for s, n in zip(ENTRY_POINTS, (9, 35)):
        assert len(getattr(lib, s).argtypes) == n
        proto = src[src.index(f"ROMAN_API int {s}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        assert "[REF roman/align/submap_align.py:108-115]" in src[:src.index(f"ROMAN_API int {s}(")].rsplit("/*", 1)[1], s
    tail = src[src.index("ROMAN_API int roman_align_lc_batch_ids("):]
    tail = " ".join(tail[:tail.index(");")].split())
    assert tail.endswith("const int64_t* ids, int32_t* n1_kept, int32_t* n2_kept, int32_t* keep")


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    assert lib.roman_shared_ids_dev(None, 0, None, None, None, None, None, None, None) != 0
    args = [None] * 35
    args[2] = 0; args[4] = 0; args[9] = 0; args[13] = 0; args[23] = 0; args[26] = 0
    assert lib.roman_align_lc_batch_ids(*args) != 0


def test_grid_form_packs_every_submap_once_and_makes_one_call(tmp_path):
    """single_robot_fill through submap_align_grid's DEFAULT compute on a stub runtime: registration.pack is called once per
    submap (the per-pair removal packs two reduced lists per pair), one batched call reaches the runtime, and every result
    equals submap_align()'s on the same submaps — the state they are left in included."""
    params, io, submaps, trajs = tsa.build("single_robot_fill")
    assert params.single_robot_lc
    params.single_robot_lc_time_thresh = 120.0               # some pairs with enough associations fall inside the time gate
    io.lc_association_thresh = 3
    S0, S1 = len(submaps[0]), len(submaps[1])
    sub_old, sub_new = copy.deepcopy(submaps), copy.deepcopy(submaps)
    old = sa.submap_align(params, sub_old, io, compute=tsa.oracle_compute)
    reg = params.get_object_registration()
    stub = si.StubIdsContext(reg); reg.set_context(stub)
    packed = []
    orig = reg.pack
    reg.pack = lambda m: (packed.append(len(m)), orig(m))[1]
    new = sa.submap_align_grid(params, sub_new, io, registration=reg)
    B = int(np.count_nonzero(~np.isnan(old.T_ij_mat[:, :, 0, 0])))
    assert B == S0 * S1
    assert len(packed) <= S0 + S1, f"registration.pack was called {len(packed)} times for {S0} + {S1} submaps ({B} pairs)"
    assert [c[:2] for c in stub.calls] == [("align_lc_batch_ids", B)]
    assert stub.calls[0][2] == sum(len(s) for r in submaps for s in r)            # the pool holds every submap once
    assert_same_state(submap_state(sub_old), submap_state(sub_new))
    for k in ["robots_nearby_mat", "clipper_num_associations", "submap_yaw_diff_mat", "T_ij_mat", "T_ij_hat_mat", "clipper_dist_mat", "clipper_angle_mat"]:
        assert np.array_equal(np.isnan(getattr(old, k)), np.isnan(getattr(new, k))), k
    np.testing.assert_array_equal(old.clipper_num_associations, new.clipper_num_associations)
    for k, tol in (("robots_nearby_mat", tsa.TOL), ("submap_yaw_diff_mat", tsa.TOL), ("T_ij_mat", tsa.TOL), ("T_ij_hat_mat", tsa.TOL),
                   ("clipper_dist_mat", 1e-7), ("clipper_angle_mat", 1e-5)):
        np.testing.assert_allclose(getattr(new, k), getattr(old, k), rtol=0, atol=tol, equal_nan=True, err_msg=k)
    shared_somewhere = False
    for i in range(S0):
        for j in range(S1):
            a, b = np.asarray(old.associated_objs_mat[i][j]).reshape(-1, 2), np.asarray(new.associated_objs_mat[i][j]).reshape(-1, 2)
            assert np.array_equal(a, b), (i, j)              # indices into the REDUCED lists
            shared_somewhere |= bool({s.id for s in submaps[0][i].segments} & {s.id for s in submaps[1][j].segments})
    assert shared_somewhere
    e_old, e_new = sa.loop_closure_edges(old, sub_old), sa.loop_closure_edges(new, sub_new)
    assert [(i, j) for i, j, _ in e_old] == [(i, j) for i, j, _ in e_new] and len(e_old) > 0
    for (_, _, Ta), (_, _, Tb) in zip(e_old, e_new):
        np.testing.assert_allclose(Tb, Ta, rtol=0, atol=tsa.TOL)
    dt = np.abs(np.array([[a.time - b.time for b in submaps[1]] for a in submaps[0]]))
    assert ((old.clipper_num_associations >= 3) & (dt < 120.0)).any()             # the time gate really stopped an edge
    assert_same_state(submap_state(sub_old), submap_state(sub_new))


def test_fallbacks_keep_the_per_pair_form():
    """An injected compute, and ids int64 cannot hold, keep today's per-pair removal (2 B packed lists, the plain entry)."""
    params, io, submaps, _ = tsa.build("single_robot_fill")
    reg = params.get_object_registration()
    stub = si.StubIdsContext(reg); reg.set_context(stub)
    calls = []
    import _lc_tail as lt
    sa.submap_align_grid(params, copy.deepcopy(submaps), io, registration=reg, compute=lambda r, b, lc: (calls.append(len(b)), lt.oracle_lc_compute(r, b, lc))[1])
    assert calls == [9] and stub.calls == []
    odd = copy.deepcopy(submaps)
    odd[0][0].segments[0].id = 2 ** 63                       # an integer, but not an int64
    res = sa.submap_align_grid(params, odd, io, registration=reg)
    assert [c[:2] for c in stub.calls] == [("align_lc_batch", 9)] and stub.calls[0][2] > sum(len(s) for r in submaps for s in r)
    named = copy.deepcopy(submaps)
    for r in named:
        for sm in r:
            for s in sm.segments:
                s.id = f"seg{s.id}"                          # ids of another type altogether
    stub.calls.clear()
    res2 = sa.submap_align_grid(params, named, io, registration=reg)
    assert [c[:2] for c in stub.calls] == [("align_lc_batch", 9)]
    assert sa._int64_ids([[si.Seg(np.int64(-5)), si.Seg(7)], []]).tolist() == [-5, 7] and sa._int64_ids([[si.Seg(1.0)]]) is None
    assert res.clipper_num_associations.shape == res2.clipper_num_associations.shape == (3, 3)
