"""The loop-closure path through the library on the GPU: submap_align_grid with the default compute against the reference
fixture; roman_align_lc_batch against roman_align_batch + the NumPy tail (tests/_lc_tail.py); a chunked batch whose first
calls skip problems for workspace — every record built from the re-issued result; roman_align_lc_batch_dev with three calls in
flight at pipeline depth 3 equal to depth 1."""
import numpy as np
import pytest

import _lc_tail as lt
from _hipmem import Hip
from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import SubmapAlignParams, batch as rb
from roman_amd.align import submap_align as sa
from roman_amd.runtime import Context, LcInputs, lc_record_dtype
from test_submap_align_grid_cpu import check_scenario_grid, compare_with_pair_loop

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(synth.ALIGN_SCENARIOS))
def test_grid_form_on_hip_matches_reference_fixture(name, tmp_path):
    check_scenario_grid(name, None, tmp_path)            # default compute: one roman_align_lc_batch call


def random_lc(B, rng, S0=None, S1=None, thresh=5):
    """Tail inputs for an arbitrary batch: reference transforms, an enable mask, frame pools."""
    from scipy.spatial.transform import Rotation as Rot
    def rigid(n, tilt):
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, :3, :3] = Rot.from_euler('ZYX', np.stack([rng.uniform(-3, 3, n), rng.normal(0, tilt, n), rng.normal(0, tilt, n)], axis=1)).as_matrix()
        T[:, :3, 3] = rng.uniform(-5, 5, (n, 3))
        return T
    S0 = S0 or 7; S1 = S1 or 5
    return LcInputs(dim=3, force_rm_upside_down=True, force_rm_lc_roll_pitch=True, lc_association_thresh=thresh, T_ref=rigid(B, 0.0),
                    enable=(rng.uniform(size=B) < 0.8).astype(np.int32), FL=rigid(S0, 0.05), iL=rng.integers(0, S0, B), FR=rigid(S1, 0.05), iR=rng.integers(0, S1, B))


def assert_lc_equals_batch_plus_numpy_tail(got, want_batch, lc):
    B = len(want_batch.assoc)
    assert np.array_equal(got.status, want_batch.status)
    for b in range(B):
        assert np.array_equal(got.assoc[b], want_batch.assoc[b]), b
    assert np.array_equal(got.T, want_batch.T, equal_nan=True)                # the same kernels in the same order
    want = lt.as_lc_result(want_batch, lc)
    lt.assert_records_match(got.records, got.accepted, want.records, want.accepted)


def test_align_lc_batch_config3_style(ctx):
    """64 pairs of 200 x 200 objects with 512-d descriptors."""
    reg = registration_for("semanticgrav", semantics_dim=512); reg.set_context(ctx)
    pairs = [synth.make_pair(200, 200, 512, 6100 + k, tilt_deg=2.0 if k % 3 else 0.0) for k in range(64)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    lc = random_lc(64, np.random.default_rng(1), thresh=40)
    lc.T_ref = np.stack([p.T_gt for p in pairs])                               # the planted transforms: small errors
    want = rb.run_batch(reg, batch)
    got = rb.run_lc_batch(reg, batch, lc)
    assert_lc_equals_batch_plus_numpy_tail(got, want, lc)
    good = (got.records["flags"] & _abi.ROMAN_LC_FAILED) == 0
    assert 0 < len(got.accepted) < 64 and good.sum() > 32 and np.max(got.records["dist"][good]) < 1.0


def test_align_lc_batch_demo_scale_grid(ctx, tmp_path):
    """A 16 x 16 grid of submaps of 20-40 objects with 768-d descriptors, method 'roman': the batch call with the tail, and
    the whole grid form against the pair loop on the same device."""
    params = SubmapAlignParams(method="roman", semantics_dim=768)
    reg = params.get_object_registration(); reg.set_context(ctx)
    rng = np.random.default_rng(2)
    subs, poses = [], []
    for s in range(32):
        m, pz = synth.make_submap_grid(1, n=int(rng.integers(20, 41)), d=768, seed0=8000 + s, overlap=0.6)
        subs.append(m[0]); poses.append(pz[0])
    common, _ = synth.make_submap_grid(32, n=30, d=768, seed0=8100, overlap=0.6)          # submaps that really overlap
    submaps = [[sa.Submap(id=k, time=400.0 * r + 20.0 * k, segments=(common if k % 2 else subs)[16 * r + k],
                          pose_flu=poses[16 * r + k] @ synth.yaw_transform(0.0, [0, 0, 0], roll=rng.normal(0, 0.02), pitch=rng.normal(0, 0.02)))
                for k in range(16)] for r in range(2)]
    batch = rb.batch_from_submap_grid(reg, [s.segments for s in submaps[0]], [s.segments for s in submaps[1]])
    assert len(batch) == 256
    lc = random_lc(256, rng, 16, 16, thresh=4); lc.iL, lc.iR = batch.pair_index[:, 0], batch.pair_index[:, 1]
    want = rb.run_batch(reg, batch)
    got = rb.run_lc_batch(reg, batch, lc)
    assert_lc_equals_batch_plus_numpy_tail(got, want, lc)
    assert len(got.accepted) > 0
    io = sa.SubmapAlignIO(lc_association_thresh=4)
    params.submap_radius = 1e3
    compare_with_pair_loop(params, io, submaps, None, tmp_path, old_compute=None, new_compute=None, registration=reg)


def test_chunked_batch_with_skipped_first_calls(monkeypatch):
    """More problems than a call holds, a fresh context (no sizing history) and a matrix pool too small for the first calls
    (ROMAN_TEST_CAPNNZ): align_chunked issues the skipped problems again BEFORE the tail runs — no record is built from a skipped
    attempt's sentinel."""
    reg = registration_for("semanticgrav", semantics_dim=16)
    pairs = [synth.make_pair(22 + (7 * k) % 19, 20 + (5 * k) % 23, 16, 9300 + k, tilt_deg=1.0) for k in range(150)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    lc = random_lc(150, np.random.default_rng(3), thresh=6)
    c = Context(0)
    try:
        reg.set_context(c); c.set_host_batching(100000, 1)
        want = rb.run_batch(reg, batch)
    finally:
        c.close()
    monkeypatch.setenv("ROMAN_TEST_CAPNNZ", "3000")
    c = Context(0)
    try:
        reg.set_context(c); c.set_host_batching(32, 3)
        got = rb.run_lc_batch(reg, batch, lc)
        assert c.skipped() > 0, "the test hook did not make the first calls overflow"
    finally:
        c.close()
    assert not np.any(got.records["flags"] & (_abi.ROMAN_LC_SKIPPED | _abi.ROMAN_LC_INTERNAL))
    assert not (got.status & _abi.ROMAN_ST_WORKSPACE).any()
    assert_lc_equals_batch_plus_numpy_tail(got, want, lc)
    assert len(got.accepted) > 10


def test_three_calls_in_flight_at_depth_3_equal_depth_1(ctx):
    """roman_align_lc_batch_dev: the tail rides on the internal stream of its batch call; three calls in flight with distinct
    output buffers give what the same calls give one after the other at depth 1."""
    reg = registration_for("semanticgrav", semantics_dim=32); reg.set_context(ctx)
    P = reg._abi_params(); F = P.feature_dim()
    hip = Hip()
    batches, lcs = [], []
    for g in range(3):
        pairs = [synth.make_pair(40 + 5 * g, 35 + 3 * k, 32, 700 + 10 * g + k) for k in range(20 + 7 * g)]
        batches.append(rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs]))
        lcs.append(random_lc(len(batches[-1]), np.random.default_rng(40 + g), thresh=8))
    for b in batches:                                            # a sizing history, so that no call skips a problem
        rb.run_batch(reg, b)

    def run(depth):
        outs = []
        for b, lc in zip(batches, lcs):
            B, kmax = len(b), b.kmax()
            T_ref, enable, FL, iL, FR, iR = lc.arrays(B)
            outs.append(dict(feats=hip.upload(b.feats), assoc=hip.alloc(B * kmax * 2 * 4), n=hip.alloc(B * 4), T=hip.alloc(B * 16 * 8), status=hip.alloc(B * 4),
                             rec=hip.alloc(B * _abi.LC_RECORD_NBYTES), idx=hip.alloc(B * 4), cnt=hip.upload(np.array([-1], np.int32)),
                             T_ref=hip.upload(T_ref), enable=hip.upload(enable), FL=hip.upload(FL), iL=hip.upload(iL), FR=hip.upload(FR), iR=hip.upload(iR)))
        ctx.set_pipeline(depth)
        try:
            for b, lc, o in zip(batches, lcs, outs):             # all three issued without waiting in between
                ctx.align_lc_batch_dev(P, o["feats"], F, b.off1, b.n1, b.off2, b.n2, b.kmax(), o["assoc"], o["n"], o["T"], o["status"],
                                       lc.params(), o["rec"], o["idx"], o["cnt"], T_ref_ptr=o["T_ref"], enable_ptr=o["enable"],
                                       FL_ptr=o["FL"], iL_ptr=o["iL"], FR_ptr=o["FR"], iR_ptr=o["iR"])
            ctx.sync()
        finally:
            ctx.set_pipeline(1)
        res = []
        for b, o in zip(batches, outs):
            B = len(b)
            cnt = int(hip.download(o["cnt"], (1,), np.int32)[0])
            res.append((hip.download(o["rec"], (B,), lc_record_dtype()), hip.download(o["idx"], (B,), np.int32)[:cnt],
                        hip.download(o["status"], (B,), np.int32), hip.download(o["n"], (B,), np.int32), hip.download(o["T"], (B, 16), np.float64)))
        return res
    try:
        one, three = run(1), run(3)
    finally:
        hip.free_all()
    for (r1, a1, s1, n1, T1), (r3, a3, s3, n3, T3), lc in zip(one, three, lcs):
        assert not (s1 & _abi.ROMAN_ST_WORKSPACE).any()
        assert np.array_equal(s1, s3) and np.array_equal(n1, n3) and np.array_equal(T1, T3, equal_nan=True)
        assert r1.tobytes() == r3.tobytes() and np.array_equal(a1, a3)         # the same kernels on the same inputs: the same bits
        want, want_acc = lt.lc_tail(lc, T1.reshape(-1, 4, 4), n1, s1)
        lt.assert_records_match(r3, a3, want, want_acc)
        assert len(a3) > 0
