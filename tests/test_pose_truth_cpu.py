"""tests/golden/pose_truth.npz without a GPU: the float64 reference restatement (oracle.t_align) stays within K / 4 of the mpmath
truth on every determined case — the condition under which K (tests/_pose_truth.py) bounds the device with a margin of 4 —, the
fixture is consistent with itself, and, where mpmath imports, three cases are evaluated again and compared bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import _pose_truth as pt
from oracle import oracle as orc

CASES = pt.load()
DET = [c for c in CASES if c["kind"] == pt.DETERMINED]
FITTED = [c for c in CASES if c["kind"] != pt.INSUFFICIENT]
#: the families of the fixture and how many cases each holds (counts at the window edges: 11, far: 2 x 3 + 1, scale: 4, flat: 4 + the
#: exact plane, needle: 2, equal / exact structure: 5, reflection: 3, 2-D: 5 + 3, undetermined: 5 + 3 past the window, k < dim entries: 7 + 5)
FAMILY_COUNTS = {"window": 11, "far": 7, "scale": 4, "flat": 5, "needle": 2, "equal": 5, "reflect": 3, "2d": 8, "undetermined": 8,
                 "batch": 12}


def test_reference_restatement_is_within_a_quarter_of_K_of_the_truth():
    worst = (0.0, None)
    for c in DET:
        T = orc.t_align(c["p1"], c["p2"], c["dim"])
        d = c["dim"]
        eR, et = pt.determined_errors(c, T[:d, :d], T[:d, d])
        print(f"{c['tag']:26s} eR = {eR:9.3g}  et = {et:9.3g}   (kappa {c['kappa']:.3g}, c/r {c['c'] / c['r']:.3g})")
        worst = max(worst, (max(eR, et), c["tag"]))
    print(f"largest: {worst[0]:.2f} at {worst[1]}; K / 4 = {pt.K / 4}")
    assert worst[0] <= pt.K / 4, worst


def test_families_and_counts():
    fam = {}
    for c in CASES:
        fam[c["family"]] = fam.get(c["family"], 0) + 1
    assert fam == FAMILY_COUNTS
    tags = [c["tag"] for c in CASES]
    assert len(set(tags)) == len(tags)
    assert [c["k"] for c in CASES if c["family"] == "window"] == [3, 4, 63, 64, 65, 127, 128, 129, 192, 193, 1000]
    assert max(c["k"] for c in CASES if c["family"] != "window") <= 200
    for c in CASES:
        assert (c["kind"] == pt.INSUFFICIENT) == (c["k"] < c["dim"]) == (c["family"] == "batch"), c["tag"]
        assert (c["kind"] == pt.UNDETERMINED) == (c["family"] == "undetermined"), c["tag"]
    for dim in (2, 3):                                             # k = 0 opens and closes each batch; k = 0, 1 (and 2) sit inside it
        ks = [c["k"] for c in CASES if c["dim"] == dim]
        assert ks[0] == 0 and ks[-1] == 0
        assert set(range(dim)) <= {k for k in ks[1:-1]}
    assert os.path.getsize(os.path.join(pt.GOLDEN, "pose_truth.npz")) < 200 * 1024


def test_fixture_is_self_consistent():
    for c in FITTED:
        orth, det = pt.properness(c["R"])
        assert orth <= 4 and det <= 4, c["tag"]                    # R* is a proper rotation rounded entry by entry
        assert np.all(np.diff(c["sv"]) <= 0) and np.all(c["sv"] >= 0), c["tag"]
        res = np.linalg.norm(c["p2"] @ c["R"].T + c["t"] - c["p1"])
        assert abs(res - c["res"]) <= 8 * pt.EPS * c["c"] * np.sqrt(c["k"]), (c["tag"], res, c["res"])
        assert c["sgn"] in (-1, 0, 1) and c["c"] == max(np.abs(c["p1"]).max(), np.abs(c["p2"]).max())
        assert np.allclose(c["m1"], c["p1"].mean(axis=0), rtol=1e-13, atol=1e-13 * c["c"])
        if c["kind"] == pt.DETERMINED:
            d, s = c["dim"], c["sv"]
            kappa = s[0] / (s[1] + c["sgn"] * s[2]) if d == 3 else max(1.0, s[0] / (s[0] + c["sgn"] * s[1]))
            assert c["kappa"] == kappa and np.isfinite(kappa) and kappa >= 0.5, c["tag"]
            assert np.allclose(c["t"], c["m1"] - c["R"] @ c["m2"], rtol=0, atol=8 * pt.EPS * c["c"])
        else:
            assert np.isnan(c["kappa"])
    by = {c["tag"]: c for c in CASES}
    assert by["axes6_reflected"]["sgn"] == -1 and all(by[f"reflect_k{k}"]["sgn"] == -1 for k in (4, 50, 129)) and by["reflect2d_k20"]["sgn"] == -1
    assert np.array_equal(by["axes6_reflected"]["R"], np.diag([-1.0, 1.0, -1.0]))       # gives up the smallest direction, not the mirrored one
    assert np.array_equal(by["axes6_pi"]["R"], np.diag([-1.0, -1.0, 1.0])) and np.array_equal(by["cube_identity"]["R"], np.eye(3))
    assert by["planar_tilted"]["sv"][2] <= 1e-60 and by["planar_tilted"]["H"].all()     # an exact null vector off the axes


def test_truth_regenerates_bit_for_bit():
    """One case at the window edge, one far from the origin, one reflection: evaluated again with mpmath from the stored points."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_pose_truth", os.path.join(pt.GOLDEN, "make_pose_truth.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    by = {c["tag"]: c for c in CASES}
    for tag in ("window_k129", "far_k129_off1e+05", "reflect_k50"):
        c = by[tag]; d = c["dim"]
        tr = gen.truth(c["p1"], c["p2"], d)
        for name in ("m1", "m2", "sv", "t"):
            assert np.array_equal(tr[name][:d], c[name]), (tag, name)
        for name in ("H", "R"):
            assert np.array_equal(tr[name][:d, :d], c[name]), (tag, name)
        assert tr["res"] == c["res"] and tr["r"] == c["r"] and tr["sgn"] == c["sgn"], tag
        assert gen.kappa_of(tr["sv"], tr["sgn"], d) == c["kappa"], tag
    assert gen.FAMILY_COUNTS == FAMILY_COUNTS
