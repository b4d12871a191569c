"""The C-ABI boundary of the segment clustering (include/roman_hip.h) without a GPU: exported and declared
symbols, the struct against the header, every argument error with its text — the argument checks run before the context is looked
at, so a NULL context reaches each of them and leaves the text with roman_last_error(NULL) — and the refusals of the Python layer
before any context exists."""
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
from roman_amd.map import ClusterParams, cluster_labels, final_cleanup, retire
from roman_amd.runtime import cluster_params, cluster_slots

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = {"roman_segment_cluster_dev": 15, "roman_segment_cluster": 13, "roman_ctx_set_cluster_cuts": 3}
CONSTS = ("ROMAN_CLUSTER_MIN_POINTS", "ROMAN_CLUSTER_WAVE_MAX", "ROMAN_CLUSTER_LDS_MAX", "ROMAN_CLUSTER_TILE", "ROMAN_CLUSTER_COLS")


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
    doc = src[src.index("roman_segment_cluster_dev (DESIGN.md"):]
    doc = doc[:doc.index("#define ROMAN_CLUSTER_MIN_POINTS")]
    assert "[REF roman/object/segment.py:195-220]" in doc and "[REF roman/map/mapper.py:92-105]" in doc and "UNPINNED" in doc
    for what in ("THE ROUNDING OF d2", "THE STRICT RADIUS COMPARISON", "THE CLOSED FORM OF THE LABEL ORDER"):
        assert what in doc, what


def test_struct_layout_matches_c(tmp_path):
    cls, name = _abi.RomanClusterParams, "roman_cluster_params_t"
    body = f'printf("{name} %zu\\n", sizeof({name}));\n'
    body += "\n".join(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_) + "\n"
    consts = "\n".join(f'printf("{k} %d\\n", {k});' for k in CONSTS)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n{body}\n{consts}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [f for f, _ in cls._fields_] == ["eps", "min_points"]
    assert int(out[name]) == C.sizeof(cls) == _abi.CLUSTER_PARAMS_NBYTES == 16
    for f, _ in cls._fields_:
        assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, f
    for k in CONSTS:
        assert int(out[k]) == getattr(_abi, k), k
    src = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert f"constexpr int CLUS_WAVE_MAX = {_abi.ROMAN_CLUSTER_WAVE_MAX};" in src and f"constexpr int CLUS_LDS_CAP = {_abi.ROMAN_CLUSTER_LDS_MAX};" in src
    assert f"constexpr int CLUS_TILE = {_abi.ROMAN_CLUSTER_TILE};" in src and f"constexpr int CLUS_COLS = {_abi.ROMAN_CLUSTER_COLS};" in src


class Call:
    """A well-formed host-pointer call over three clouds and two jobs, one argument at a time made wrong."""
    def __init__(self):
        self.P = cluster_params(0.25, 10)
        self.points = np.zeros((9, 3)); self.off = np.array([0, 4, 6, 9], dtype=np.int64); self.n_clouds = 3
        self.jobs = np.array([2, 0], dtype=np.int32); self.n_jobs = 2
        self.out_points = np.zeros((7, 3)); self.count = np.zeros(2, np.int32); self.status = np.zeros(2, np.int32)
        self.labels = np.zeros(7, np.int32); self.n_clusters = np.zeros(2, np.int32); self.kept = np.zeros(2, np.int32)

    def run(self, lib, dev):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        head = (None, C.byref(self.P) if self.P is not None else None, p(self.points))
        tail = (self.n_jobs, p(self.out_points), p(self.count), p(self.status), p(self.labels), p(self.n_clusters), p(self.kept))
        if dev:                                             # nothing is dereferenced on the device side before the context check
            return lib.roman_segment_cluster_dev(*head, p(self.off), p(self.off), self.n_clouds, p(self.jobs), p(self.jobs), *tail)
        return lib.roman_segment_cluster(*head, p(self.off), self.n_clouds, p(self.jobs), *tail)


def setp(name, value):
    return lambda c: setattr(c.P, name, value)


def setj(k, value):
    def f(c):
        c.jobs[k] = value
    return f


NULLS = "out_points / out_count / out_status / out_n_clusters is NULL"
ERRORS = [
    ("params is NULL", lambda c: setattr(c, "P", None)),
    ("eps must be finite and > 0", setp("eps", 0.0)),
    ("eps must be finite and > 0", setp("eps", -0.25)),
    ("eps must be finite and > 0", setp("eps", float("inf"))),
    ("eps must be finite and > 0", setp("eps", float("nan"))),
    ("min_points must be >= 1 (got 0)", setp("min_points", 0)),
    ("min_points must be >= 1 (got -3)", setp("min_points", -3)),
    ("n_clouds = -1, n_jobs = 2", lambda c: setattr(c, "n_clouds", -1)),
    ("n_clouds = 3, n_jobs = -1", lambda c: setattr(c, "n_jobs", -1)),
    ("cloud_off is NULL", lambda c: setattr(c, "off", None)),
    ("cloud_off[0] = 1: the first cloud starts at row 0", lambda c: setattr(c, "off", np.array([1, 4, 6, 9], dtype=np.int64))),
    ("cloud_off descends at cloud 1", lambda c: setattr(c, "off", np.array([0, 6, 4, 9], dtype=np.int64))),
    ("jobs is NULL", lambda c: setattr(c, "jobs", None)),
    ("job 0: 3 is not one of the 3 clouds", setj(0, 3)),
    ("job 1: -1 is not one of the 3 clouds", setj(1, -1)),
    ("job 1: cloud 2 is named by an earlier job", setj(1, 2)),
    ("points is NULL", lambda c: setattr(c, "points", None)),
    (NULLS, lambda c: setattr(c, "out_points", None)),
    (NULLS, lambda c: setattr(c, "count", None)),
    (NULLS, lambda c: setattr(c, "status", None)),
    (NULLS, lambda c: setattr(c, "n_clusters", None)),
    ("ctx is NULL", lambda c: None),
    ("ctx is NULL", lambda c: (setattr(c, "labels", None), setattr(c, "kept", None))),                  # the optional outputs
    ("ctx is NULL", lambda c: setp("min_points", 1)(c)),                                                # a run-time value
    ("ctx is NULL", lambda c: (setattr(c, "off", np.zeros(4, np.int64)), setattr(c, "points", None), setattr(c, "out_points", None))),   # every slot empty
    ("ctx is NULL", lambda c: setattr(c, "n_jobs", 0)),                                                 # the context is looked at last, then ROMAN_OK
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
    c.off = np.array([0, 4, 6, 2**31 + 6], dtype=np.int64)
    assert c.run(lib, False) == _abi.ROMAN_E_TOO_LARGE and b"cloud 2 holds more than" in lib.roman_last_error(None)
    c = Call()
    c.off = np.array([0, 4, 6, 2**28 + 3], dtype=np.int64)          # 2^28 - 3 points in cloud 2 and 4 in cloud 0: one past 2^28
    assert c.run(lib, True) == _abi.ROMAN_E_TOO_LARGE and b"the jobs hold more than 2^28 points" in lib.roman_last_error(None)
    c.off = np.array([0, 4, 6, 2**28 + 2], dtype=np.int64)          # exactly 2^28: the checks pass, the context is missing
    assert c.run(lib, True) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)
    assert lib.roman_ctx_set_cluster_cuts(None, 0, 0) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_builds_the_blocks_the_header_describes():
    P = cluster_params()
    assert (P.eps, P.min_points) == (0.25, 10)
    a = ClusterParams.from_mapper_params(SimpleNamespace(clustering_epsilon=0.25))
    assert a == ClusterParams() and a.abi().eps == 0.25 and a.abi().min_points == 10
    assert ClusterParams(0.4, 3).abi().min_points == 3
    assert cluster_slots([0, 4, 6, 9, 9], [2, 0, 3]).tolist() == [0, 3, 7, 7]
    assert cluster_slots([0, 4], []).tolist() == [0]


def clouds(sizes, d=None, seed=0):
    rng = np.random.default_rng(seed)
    obs = [SimpleNamespace(transformed_points=rng.normal(size=(n, 3)), time=1.0 + i, semantic_descriptor=None if d is None else rng.normal(size=d))
           for i, n in enumerate(sizes)]
    return SegmentClouds.from_observations(obs)


def test_refusals_come_before_any_context(monkeypatch):
    """Every refusal is a ValueError raised while NO context exists: the default context is replaced by a function that fails,
    and the context handed in refuses every attribute that is asked of it."""
    import roman_amd.runtime as rt

    def no_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(rt, "default_context", no_context)
    monkeypatch.setattr(rt, "Context", no_context)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the context was asked for {name} before the refusal")

    S, P = clouds([5, 6, 7], 8), ClusterParams()
    bad_params = [dataclasses.replace(P, clustering_epsilon=e) for e in (0.0, -0.25, float("inf"), float("nan"))]
    bad_params += [dataclasses.replace(P, min_points=m) for m in (0, -1, 2.5)]
    for ctx in (Untouchable(), None):
        for p in bad_params:
            with pytest.raises(ValueError):
                p.abi()
            with pytest.raises(ValueError):
                final_cleanup(S, [0], p, ctx=ctx)
            with pytest.raises(ValueError):
                cluster_labels(np.zeros((4, 3)), p, ctx=ctx)
            with pytest.raises(ValueError):
                retire(S, 10.0, None, 1.0, p, ctx=ctx)
        for which in ([3], [-1], [1, 1]):
            with pytest.raises(ValueError):
                final_cleanup(S, which, P, ctx=ctx)
        with pytest.raises(ValueError):
            final_cleanup(dataclasses.replace(S, points=S.points[:, :2]), [0], P, ctx=ctx)
        with pytest.raises(ValueError):
            cluster_labels(np.zeros((4, 2)), P, ctx=ctx)
        with pytest.raises(ValueError):
            retire(S, 10.0, np.zeros(2), 1.0, P, ctx=ctx)
        # nothing to do: an empty answer, and still no context
        r = final_cleanup(S, [], P, ctx=ctx)
        assert len(r.clouds) == 0 and r.dropped.shape == (0,) and r.clouds.descriptors.shape == (0, 8) and r.kept.shape == (0,)
        assert cluster_labels(np.zeros((0, 3)), P, ctx=ctx).shape == (0,)
        active, inactive, dropped = retire(S, 2.0, None, 5.0, P, ctx=ctx)      # every segment was seen recently enough
        assert active.tolist() == [0, 1, 2] and len(inactive) == 0 and dropped.shape == (0,)
