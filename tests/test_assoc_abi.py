"""The C-ABI boundary of the association scores (include/roman_hip.h) without a GPU: exported and declared
symbols, the struct against the header, every argument error with its text — the argument checks run before the context is
looked at, so a NULL context reaches each of them and leaves the text with roman_last_error(NULL) — and the refusals of the
Python layer before any context exists."""
import ctypes as C
import dataclasses
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from roman_amd import _abi
from roman_amd.align import SegmentClouds
from roman_amd.map import AssociationParams, association_scores, global_nearest_neighbor
from roman_amd.map.association import pairs_from_scores
from roman_amd.runtime import assoc_params

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = {"roman_assoc_scores_dev": 15, "roman_assoc_scores": 14, "roman_ctx_set_assoc_cuts": 3}
CONSTS = ("ROMAN_ASSOC_IOU", "ROMAN_ASSOC_IOM", "ROMAN_ASSOC_OK", "ROMAN_ASSOC_EMPTY", "ROMAN_ASSOC_RANGE", "ROMAN_ASSOC_WAVE_MAX", "ROMAN_ASSOC_LDS_MAX")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, nargs in ENTRY_POINTS.items():
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        proto = src[src.index(f"ROMAN_API int {s}("):]
        assert proto[:proto.index(");")].count(",") + 1 == nargs, s
    assert "[REF roman/map/global_nearest_neighbor.py:23-36]" in src and "[REF roman/map/voxel_grid.py:32-103]" in src
    assert "UNPINNED" in src[src.index("roman_assoc_scores_dev (DESIGN.md"):]


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.RomanAssocParams._fields_]
    assert fields == ["voxel_size", "geometric", "semantic", "geo_range", "sem_range"]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(roman_assoc_params_t, {f}));' for f in fields)
    consts = "\n".join(f'printf("{k} %d\\n", {k});' for k in CONSTS)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof %zu\\n", sizeof(roman_assoc_params_t));\n{body}\n{consts}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == C.sizeof(_abi.RomanAssocParams) == _abi.ASSOC_PARAMS_NBYTES == 48
    for f in fields:
        assert int(out[f]) == getattr(_abi.RomanAssocParams, f).offset, f
    for k in CONSTS:
        assert int(out[k]) == getattr(_abi, k), k
    src = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert f"constexpr int ASSOC_WAVE_MAX = {_abi.ROMAN_ASSOC_WAVE_MAX};" in src and f"constexpr int ASSOC_LDS_CAP = {_abi.ROMAN_ASSOC_LDS_MAX};" in src


class Call:
    """A well-formed host-pointer call over 2 + 1 clouds, one argument at a time made wrong."""
    def __init__(self):
        self.P = assoc_params(0.2, "iou", True)
        self.points = np.zeros((6, 3)); self.off = np.array([0, 2, 4, 6], dtype=np.int64)
        self.N1, self.N2, self.d = 2, 1, 4
        self.desc = np.ones((3, 4))
        self.n_vox = np.zeros(3, np.int32); self.status = np.zeros(3, np.int32); self.inter = np.zeros(2, np.int32)
        self.geo = np.zeros(2); self.sem = np.zeros(2); self.score = np.zeros(2)

    def run(self, lib, dev):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        head = (None, C.byref(self.P) if self.P is not None else None, p(self.points))
        tail = (self.N1, self.N2, p(self.desc), self.d, p(self.n_vox), p(self.inter), p(self.geo), p(self.sem), p(self.score), p(self.status))
        if dev:                                             # nothing is dereferenced on the device side before the context check
            return lib.roman_assoc_scores_dev(*head, p(self.off), p(self.off), *tail)
        return lib.roman_assoc_scores(*head, p(self.off), *tail)


def setp(name, value):
    return lambda c: setattr(c.P, name, value)


def setr(name, lo, hi):
    def f(c):
        r = getattr(c.P, name); r[0], r[1] = lo, hi
    return f


ERRORS = [
    ("params is NULL", lambda c: setattr(c, "P", None)),
    ("voxel_size must be finite and > 0", setp("voxel_size", 0.0)),
    ("voxel_size must be finite and > 0", setp("voxel_size", -0.2)),
    ("voxel_size must be finite and > 0", setp("voxel_size", float("inf"))),
    ("voxel_size must be finite and > 0", setp("voxel_size", float("nan"))),
    ("unknown geometric method 2", setp("geometric", 2)),
    ("semantic must be 0 or 1", setp("semantic", 2)),
    ("geo_range = (0.25, 0.25): threshold and maximum must differ", setr("geo_range", 0.25, 0.25)),
    ("geo_range = (nan, 1)", setr("geo_range", float("nan"), 1.0)),
    ("sem_range = (0.8, 0.8): threshold and maximum must differ", setr("sem_range", 0.8, 0.8)),
    ("N1 = -1, N2 = 1", lambda c: setattr(c, "N1", -1)),
    ("N1 = 2, N2 = -2", lambda c: setattr(c, "N2", -2)),
    ("cloud_off is NULL", lambda c: setattr(c, "off", None)),
    ("cloud_off[0] = 1: the first cloud starts at row 0", lambda c: setattr(c, "off", np.array([1, 2, 4, 6], dtype=np.int64))),
    ("cloud_off descends at cloud 1", lambda c: setattr(c, "off", np.array([0, 4, 2, 6], dtype=np.int64))),
    ("d < 0", lambda c: setattr(c, "d", -1)),
    ("desc is NULL with d = 4", lambda c: setattr(c, "desc", None)),
    ("desc is given with d = 0", lambda c: setattr(c, "d", 0)),
    ("points is NULL", lambda c: setattr(c, "points", None)),
    ("geo / score / status is NULL", lambda c: setattr(c, "geo", None)),
    ("geo / score / status is NULL", lambda c: setattr(c, "score", None)),
    ("geo / score / status is NULL", lambda c: setattr(c, "status", None)),
    ("ctx is NULL", lambda c: None),
    ("ctx is NULL", lambda c: (setattr(c, "n_vox", None), setattr(c, "inter", None), setattr(c, "sem", None))),      # the optional outputs
    ("ctx is NULL", lambda c: (setp("semantic", 0)(c), setr("sem_range", 0.8, 0.8)(c), setattr(c, "desc", None))),  # a range and descriptors not in use
]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("k", range(len(ERRORS)))
def test_every_argument_error_has_its_text(k, dev):
    lib = _abi.load_library()
    text, wrong = ERRORS[k]
    c = Call()
    wrong(c)
    assert c.run(lib, dev) == _abi.ROMAN_E_INVALID
    assert text.encode() in lib.roman_last_error(None), lib.roman_last_error(None)


def test_too_large_and_the_cuts_hook():
    lib = _abi.load_library()
    c = Call()
    c.off = np.array([0, 2, 4, 2**31 + 4], dtype=np.int64)
    assert c.run(lib, False) == _abi.ROMAN_E_TOO_LARGE and b"cloud 2 holds more than" in lib.roman_last_error(None)
    c = Call(); c.N1, c.N2 = 2**30, 2**30
    assert c.run(lib, False) == _abi.ROMAN_E_TOO_LARGE and b"2^30 clouds" in lib.roman_last_error(None)
    assert lib.roman_ctx_set_assoc_cuts(None, 0, 0) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_builds_the_block_the_header_describes():
    P = assoc_params()
    assert (P.voxel_size, P.geometric, P.semantic, tuple(P.geo_range), tuple(P.sem_range)) == (0.2, 0, 0, (0.25, 1.0), (0.8, 1.0))
    ref_defaults = SimpleNamespace(geometric_association_method="iou", semantic_association_method=None, geometric_score_range=(0.25, 1.0),
                                   semantic_score_range=(0.8, 1.0), iou_voxel_size=0.2)
    a = AssociationParams.from_mapper_params(ref_defaults)
    assert a == AssociationParams() and not a.semantic and a.abi().semantic == 0
    for none in (None, "none", "None"):
        assert not dataclasses.replace(a, semantic_association_method=none).semantic
    b = dataclasses.replace(a, geometric_association_method="iom", semantic_association_method="cosine_similarity", iou_voxel_size=0.05).abi()
    assert (b.geometric, b.semantic, b.voxel_size) == (_abi.ROMAN_ASSOC_IOM, 1, 0.05)
    with pytest.raises(ValueError):
        assoc_params(geometric="chamfer")


def obs(n, d=None, seed=0):
    rng = np.random.default_rng(seed)
    return SimpleNamespace(transformed_points=None if n is None else rng.normal(size=(n, 3)), time=1.5 + seed,
                           semantic_descriptor=None if d is None else rng.normal(size=d))


def test_segment_clouds_from_observations():
    c = SegmentClouds.from_observations([obs(4, 8, 0), obs(None, 8, 1), obs(7, 8, 2)])
    assert len(c) == 3 and c.seg_off.tolist() == [0, 4, 4, 11] and c.points.shape == (11, 3) and c.points.dtype == np.float64
    assert c.ids.tolist() == [0, 1, 2] and c.times.tolist() == [[1.5, 1.5], [2.5, 2.5], [3.5, 3.5]] and c.descriptors.shape == (3, 8)
    assert SegmentClouds.from_observations([obs(4, 8), obs(3, None)]).descriptors is None
    e = SegmentClouds.from_observations([])
    assert len(e) == 0 and e.points.shape == (0, 3) and e.seg_off.tolist() == [0]


def test_refusals_come_before_any_context(monkeypatch):
    """Every refusal is a ValueError raised while NO context exists: the default context is replaced by a function that fails,
    and the context handed in records every attribute that is asked of it."""
    import roman_amd.runtime as rt

    def no_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(rt, "default_context", no_context)
    monkeypatch.setattr(rt, "Context", no_context)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the context was asked for {name} before the refusal")

    good = SegmentClouds.from_observations([obs(5, 8, i) for i in range(3)])
    P = AssociationParams(semantic_association_method="cosine_similarity")
    bad = [
        (good, good, dataclasses.replace(P, geometric_association_method="chamfer")),
        (good, good, dataclasses.replace(P, geometric_association_method="mask")),
        (good, good, dataclasses.replace(P, semantic_association_method="clip")),
        (good, good, dataclasses.replace(P, iou_voxel_size=0.0)),
        (good, good, dataclasses.replace(P, iou_voxel_size=float("nan"))),
        (good, good, dataclasses.replace(P, geometric_score_range=(0.5, 0.5))),
        (good, good, dataclasses.replace(P, semantic_score_range=(1.0, 1.0))),
        (good, good, dataclasses.replace(P, geometric_score_range=(0.5,))),
        (dataclasses.replace(good, points=good.points[:, :2]), good, P),
        (dataclasses.replace(good, seg_off=np.array([0, 5, 4, 15])), good, P),
        (good, dataclasses.replace(good, seg_off=np.array([0, 5, 10, 14])), P),
        (good, dataclasses.replace(good, descriptors=good.descriptors[:, :5]), P),
        (good, dataclasses.replace(good, descriptors=good.descriptors[:2]), P),
    ]
    for a, b, p in bad:
        for ctx in (Untouchable(), None):
            for fn in (association_scores, global_nearest_neighbor):
                with pytest.raises(ValueError):
                    fn(a, b, p, ctx=ctx)
    with pytest.raises(ValueError, match="chamfer.*not covered"):
        association_scores(good, None, dataclasses.replace(P, geometric_association_method="chamfer"))
    # no cloud on a side: an empty answer, and still no context
    empty = SegmentClouds.from_observations([])
    r = association_scores(empty, good, P, ctx=Untouchable())
    assert r.score.shape == (0, 3) and r.status.shape == (3,) and global_nearest_neighbor(good, empty, P, ctx=Untouchable()) == []


def test_pairs_from_scores_is_the_reference_extraction():
    M = 1e9
    assert pairs_from_scores(np.array([[-0.9, M, M], [M, M, -0.4]])) == [(0, 0), (1, 2)]
    assert pairs_from_scores(np.full((2, 3), M)) == [] and pairs_from_scores(np.zeros((0, 2))) == []
