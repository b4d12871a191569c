"""method='ransac' without a GPU: the factory and the plugin's surface, the integer sampler, and the NumPy oracle of the
deterministic procedure (tests/_ransac_oracle.py) on cases whose answer is known."""
import numpy as np
import pytest

import _ransac_oracle as ro
from roman_amd.align import RansacReg, SubmapAlignParams


def test_factory_returns_ransac_reg_with_ransac_iter():
    reg = SubmapAlignParams(method='ransac', ransac_iter=12345).get_object_registration()
    assert isinstance(reg, RansacReg)
    assert reg.max_iteration == 12345 and reg.dim == 3 and reg.edge_len == 0.95
    assert (reg.round, reg.max_dist, reg.confidence, reg.seed) == (4096, 0.5, 0.999, 0)
    assert SubmapAlignParams(method='ransac').get_object_registration().max_iteration == int(1e6)
    p = reg._ransac_params()
    assert (p.max_iteration, p.round, p.edge_len, p.max_dist, p.confidence, p.seed) == (12345, 4096, 0.95, 0.5, 0.999, 0)


def test_dim_2_trips_the_assertion():
    with pytest.raises(AssertionError, match="Only 3D"):
        RansacReg(dim=2)
    with pytest.raises(AssertionError):
        SubmapAlignParams(method='ransac', dim=2).get_object_registration()


def test_plugin_surface_without_a_device():
    reg = RansacReg(0.9, 3, 500, round=64, seed=7)
    assert (reg.edge_len, reg.max_iteration, reg.round, reg.seed) == (0.9, 500, 64, 7)
    with pytest.raises(TypeError):
        RansacReg(0.9, 3, 500, 64)                               # the extras are keyword-only
    segs = ro.segments(np.arange(12.0).reshape(4, 3))
    assert np.array_equal(reg.pack(segs), np.arange(12.0).reshape(4, 3)) and reg.pack([]).shape == (0, 3)
    assert reg.register([], segs).shape == (1, 0) and reg.register(segs, []).shape == (1, 0)     # as the base class, no device needed
    for call in (lambda: reg.get_MCA(segs, segs), lambda: reg.mno_clipper(segs, segs), lambda: reg.mno_clipper_batch([(segs, segs)])):
        with pytest.raises(NotImplementedError):
            call()


def test_grid_form_refuses_ransac_at_its_top():
    from roman_amd.align.submap_align import submap_align_grid
    with pytest.raises(NotImplementedError):
        submap_align_grid(SubmapAlignParams(method='ransac'), [[], []])


def test_draw_test_vector():
    """The first three outputs of splitmix64 seeded with 0."""
    assert [ro.draw(0, c) for c in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert ro.draw(5, 0) == ro.mix64(5 + ro.GOLDEN) and ro.draw(ro.MASK64, 0) == ro.mix64(ro.GOLDEN - 1)      # the sum wraps mod 2^64


@pytest.mark.parametrize("nm", [1, 1024 * 1024])
def test_mulhi64_indices_stay_in_range(nm):
    draws = [0, 1, ro.MASK64, ro.MASK64 - 1, 1 << 63] + [ro.draw(3, c) for c in range(2000)]
    idx = [ro.mulhi64(d, nm) for d in draws]
    assert min(idx) >= 0 and max(idx) < nm
    assert ro.mulhi64(ro.MASK64, nm) == nm - 1
    if nm > 1:
        assert len(set(idx)) > 1000                              # spread over the range, not stuck at an end
        m = 1024
        for (i, j) in ro.sample(3, 17, 1024, m):
            assert 0 <= i < 1024 and 0 <= j < m


def test_oracle_recovers_a_planted_pair(orc):
    """8 objects, 6 of them carried by a known rigid motion with 1 cm noise, 2 replaced."""
    P, Q, R, t, truth = ro.planted(8, 8, 301, n_in=6, noise=0.01)
    rows, T, res = ro.result(orc, P, Q, max_iteration=20000, round=256)
    assert res.n_border == 0 and len(res.best_set) == 1
    assert res.best_count == 6 and np.array_equal(rows, truth[np.argsort(truth[:, 0])])
    # T maps map 2 -> map 1: the inverse of the planted motion, within the noise (1 cm on points up to ~17 m from the origin)
    Tp = np.eye(4); Tp[:3, :3] = R.T; Tp[:3, 3] = -R.T @ t
    assert np.linalg.norm(T[:3, :3] - Tp[:3, :3]) < 0.01 and np.linalg.norm(T[:3, 3] - Tp[:3, 3]) < 0.1
    resid = np.linalg.norm(P[rows[:, 0]] - (Q[rows[:, 1]] @ T[:3, :3].T + T[:3, 3]), axis=1)
    assert resid.max() < 0.05


def test_stop_rule_on_whole_rounds():
    """n = m = 4, all planted: once a round has found the four true rows the estimate is ceil(log(0.001) / log(1 - (4/16)^3)) =
    439 and the problem stops at the first multiple of 64 that reaches it."""
    P, Q, _, _, _ = ro.planted(4, 4, 201)
    res = ro.run(P, Q, max_iteration=4096, round=64)
    assert res.n_border == 0
    # the oracle's own count: replay the rounds from the per-hypothesis counts
    best, done, want = -1, 0, None
    while want is None:
        done += 64
        best = max(best, int(res.counts[done - 64:done].max()))
        if done >= ro.stop_estimate(best, 16, 4096, 0.999):
            want = done
    assert res.n_hyp == want == len(res.counts)
    assert int(res.counts[:64].max()) == 4 and ro.stop_estimate(4, 16, 4096, 0.999) == 439 and res.n_hyp == 448
    assert ro.stop_estimate(0, 16, 4096, 0.999) == 4096 and ro.stop_estimate(16, 16, 4096, 0.999) == 0
    assert ro.run(P, Q, max_iteration=300, round=256).n_hyp == 300           # the last round is cut at max_iteration
