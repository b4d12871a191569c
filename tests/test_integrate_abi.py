"""The C-ABI boundary of the segment update (include/roman_hip.h) without a GPU: exported and declared symbols,
the structs against the header, every argument error with its text — the argument checks run before the context is looked at, so
a NULL context reaches each of them and leaves the text with roman_last_error(NULL) — and the refusals of the Python layer before
any context exists."""
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
from roman_amd.map import IntegrationParams, cleanup_points, integrate
from roman_amd.runtime import integrate_jobs, integrate_params, integrate_slots

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = {"roman_segment_integrate_dev": 16, "roman_segment_integrate": 14, "roman_ctx_set_integrate_cuts": 3}
CONSTS = ("ROMAN_INTEGRATE_NEIGHBORS", "ROMAN_INTEGRATE_WAVE_MAX", "ROMAN_INTEGRATE_LDS_MAX")


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
    doc = src[src.index("roman_segment_integrate_dev (DESIGN.md"):]
    assert "[REF roman/object/segment.py:98-161]" in doc and "[REF roman/object/segment.py:177-193]" in doc and doc.count("UNPINNED") >= 3


def test_struct_layout_matches_c(tmp_path):
    structs = {"roman_integrate_params_t": _abi.RomanIntegrateParams, "roman_integrate_job_t": _abi.RomanIntegrateJob}
    body = ""
    for name, cls in structs.items():
        body += f'printf("{name} %zu\\n", sizeof({name}));\n'
        body += "\n".join(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_) + "\n"
    consts = "\n".join(f'printf("{k} %d\\n", {k});' for k in CONSTS)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n{body}\n{consts}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [f for f, _ in _abi.RomanIntegrateParams._fields_] == ["voxel_size", "outlier_std", "nb_neighbors"]
    assert [f for f, _ in _abi.RomanIntegrateJob._fields_] == ["base", "add", "pose"]
    for name, cls in structs.items():
        assert int(out[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(out[f"{name}.{f}"]) == getattr(cls, f).offset, f
    assert _abi.INTEGRATE_PARAMS_NBYTES == 24 and np.dtype(_abi.INTEGRATE_JOB_DTYPE).itemsize == C.sizeof(_abi.RomanIntegrateJob) == 12
    for k in CONSTS:
        assert int(out[k]) == getattr(_abi, k), k
    src = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert f"constexpr int INTEG_WAVE_MAX = {_abi.ROMAN_INTEGRATE_WAVE_MAX};" in src and f"constexpr int INTEG_LDS_CAP = {_abi.ROMAN_INTEGRATE_LDS_MAX};" in src
    assert f"constexpr int INTEG_NEIGHBORS = {_abi.ROMAN_INTEGRATE_NEIGHBORS};" in src


class Call:
    """A well-formed host-pointer call over three clouds, two poses and two jobs, one argument at a time made wrong."""
    def __init__(self):
        self.P = integrate_params(0.05, 1.0)
        self.points = np.zeros((9, 3)); self.off = np.array([0, 4, 6, 9], dtype=np.int64); self.n_clouds = 3
        self.poses = np.tile(np.eye(4), (2, 1, 1)); self.n_poses = 2
        self.jobs = integrate_jobs([(0, 1, 0), (None, 2, None)]); self.n_jobs = 2
        self.out_points = np.zeros((9, 3)); self.count = np.zeros(2, np.int32); self.status = np.zeros(2, np.int32)
        self.avg = np.zeros(9); self.thr = np.zeros(2)

    def run(self, lib, dev):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        head = (None, C.byref(self.P) if self.P is not None else None, p(self.points))
        tail = (self.n_jobs, p(self.out_points), p(self.count), p(self.status), p(self.avg), p(self.thr))
        if dev:                                             # nothing is dereferenced on the device side before the context check
            return lib.roman_segment_integrate_dev(*head, p(self.off), p(self.off), self.n_clouds, p(self.poses), self.n_poses, p(self.jobs), p(self.jobs), *tail)
        return lib.roman_segment_integrate(*head, p(self.off), self.n_clouds, p(self.poses), self.n_poses, p(self.jobs), *tail)


def setp(name, value):
    return lambda c: setattr(c.P, name, value)


def setj(k, field, value):
    def f(c):
        c.jobs[k][field] = value
    return f


ERRORS = [
    ("params is NULL", lambda c: setattr(c, "P", None)),
    ("voxel_size must be finite and > 0", setp("voxel_size", 0.0)),
    ("voxel_size must be finite and > 0", setp("voxel_size", -0.05)),
    ("voxel_size must be finite and > 0", setp("voxel_size", float("inf"))),
    ("voxel_size must be finite and > 0", setp("voxel_size", float("nan"))),
    ("outlier_std is NaN", setp("outlier_std", float("nan"))),
    ("nb_neighbors must be 10 (got 9)", setp("nb_neighbors", 9)),
    ("nb_neighbors must be 10 (got 0)", setp("nb_neighbors", 0)),
    ("n_clouds = -1, n_poses = 2, n_jobs = 2", lambda c: setattr(c, "n_clouds", -1)),
    ("n_clouds = 3, n_poses = -1, n_jobs = 2", lambda c: setattr(c, "n_poses", -1)),
    ("n_clouds = 3, n_poses = 2, n_jobs = -1", lambda c: setattr(c, "n_jobs", -1)),
    ("cloud_off is NULL", lambda c: setattr(c, "off", None)),
    ("cloud_off[0] = 1: the first cloud starts at row 0", lambda c: setattr(c, "off", np.array([1, 4, 6, 9], dtype=np.int64))),
    ("cloud_off descends at cloud 1", lambda c: setattr(c, "off", np.array([0, 6, 4, 9], dtype=np.int64))),
    ("jobs is NULL", lambda c: setattr(c, "jobs", None)),
    ("job 0: add = 3 is not one of the 3 clouds", setj(0, "add", 3)),
    ("job 1: add = -1 is not one of the 3 clouds", setj(1, "add", -1)),
    ("job 0: base = 3 is neither -1 nor one of the 3 clouds", setj(0, "base", 3)),
    ("job 1: base = -2 is neither -1 nor one of the 3 clouds", setj(1, "base", -2)),
    ("job 0: pose = 2 is neither -1 nor one of the 2 poses", setj(0, "pose", 2)),
    ("job 1: pose = -2 is neither -1 nor one of the 2 poses", setj(1, "pose", -2)),
    ("job 1: base cloud 0 is the base of an earlier job", setj(1, "base", 0)),
    ("poses is NULL and a job names one", lambda c: setattr(c, "poses", None)),
    ("points is NULL", lambda c: setattr(c, "points", None)),
    ("out_points / out_count / out_status is NULL", lambda c: setattr(c, "out_points", None)),
    ("out_points / out_count / out_status is NULL", lambda c: setattr(c, "count", None)),
    ("out_points / out_count / out_status is NULL", lambda c: setattr(c, "status", None)),
    ("ctx is NULL", lambda c: None),
    ("ctx is NULL", lambda c: (setattr(c, "avg", None), setattr(c, "thr", None))),                      # the optional outputs
    ("ctx is NULL", lambda c: (setj(0, "pose", -1)(c), setattr(c, "poses", None))),                     # poses no job names
    ("ctx is NULL", lambda c: setp("outlier_std", float("inf"))(c)),                                    # no outlier removal
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
    c.off = np.array([0, 4, 6, 2**28 + 7], dtype=np.int64)
    assert c.run(lib, True) == _abi.ROMAN_E_TOO_LARGE and b"job 1 holds more than 2^28 points" in lib.roman_last_error(None)
    assert lib.roman_ctx_set_integrate_cuts(None, 0, 0) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_builds_the_blocks_the_header_describes():
    P = integrate_params()
    assert (P.voxel_size, P.outlier_std, P.nb_neighbors) == (0.05, 1.0, 10)
    assert integrate_params(0.1, None).outlier_std == 0.0
    ref_defaults = SimpleNamespace(segment_voxel_size=0.05, segment_outlier_removal_std=1.0)
    a = IntegrationParams.from_mapper_params(ref_defaults)
    assert a == IntegrationParams() and a.abi().voxel_size == 0.05 and a.abi().outlier_std == 1.0
    j = integrate_jobs([(0, 1), (None, 2, None), (3, 0, 1)])
    assert j.tolist() == [(0, 1, -1), (-1, 2, -1), (3, 0, 1)] and j.dtype.itemsize == 12
    assert integrate_slots([0, 4, 6, 9, 9], j).tolist() == [0, 6, 9, 13]
    with pytest.raises(ValueError):
        integrate_jobs([(0,)])


def clouds(sizes, d=None, seed=0):
    rng = np.random.default_rng(seed)
    obs = [SimpleNamespace(transformed_points=rng.normal(size=(n, 3)), time=1.0 + i, semantic_descriptor=None if d is None else rng.normal(size=d))
           for i, n in enumerate(sizes)]
    return SegmentClouds.from_observations(obs)


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

    S, A = clouds([5, 6, 7], 8, 0), clouds([4, 3], 8, 1)
    P = IntegrationParams()
    poses = np.tile(np.eye(4), (2, 1, 1))
    good = [(0, 0, 0), (None, 1, 1)]
    bad = [
        (S, A, good, dataclasses.replace(P, segment_voxel_size=0.0), poses),
        (S, A, good, dataclasses.replace(P, segment_voxel_size=float("nan")), poses),
        (S, A, good, dataclasses.replace(P, segment_outlier_removal_std=float("nan")), poses),
        (S, A, [(3, 0, 0)], P, poses),
        (S, A, [(0, 2, 0)], P, poses),
        (S, A, [(0, None, 0)], P, poses),
        (S, A, [(0, 0, 2)], P, poses),
        (S, A, [(0, 0, 0)], P, None),
        (S, A, [(1, 0), (1, 1)], P, poses),
        (S, A, [(0, 0, 0, 0)], P, poses),
        (S, A, good, P, np.eye(4)),
        (dataclasses.replace(S, points=S.points[:, :2]), A, good, P, poses),
        (S, dataclasses.replace(A, seg_off=np.array([0, 5, 4])), good, P, poses),
        (S, dataclasses.replace(A, descriptors=A.descriptors[:, :5]), good, P, poses),
    ]
    for s, a, jobs, p, T in bad:
        for ctx in (Untouchable(), None):
            with pytest.raises(ValueError):
                integrate(s, a, jobs, p, poses=T, ctx=ctx)
    for ctx in (Untouchable(), None):
        with pytest.raises(ValueError):
            cleanup_points(np.zeros((4, 3)), dataclasses.replace(P, segment_voxel_size=-1.0), ctx=ctx)
        with pytest.raises(ValueError):
            cleanup_points(np.zeros((4, 2)), P, ctx=ctx)
        # no job, no point: an empty answer, and still no context
        r = integrate(S, A, [], P, poses=poses, ctx=ctx)
        assert len(r.clouds) == 0 and r.status.shape == (0,) and r.threshold.shape == (0,) and r.clouds.descriptors.shape == (0, 8)
        assert cleanup_points(np.zeros((0, 3)), P, ctx=ctx).shape == (0, 3)


def test_descriptor_update_is_the_references_with_its_renormalisation():
    """roman_amd.map.update._descriptor against tests/_integrate_oracle.Descriptor — _add_semantic_descriptor line by line, the
    renormalisation behind both branches included — over a chain of updates and a merge with a count above one: identical bits
    at every step, unit norm at every step, and NOT the mean without the renormalisation."""
    import _integrate_oracle as io
    from roman_amd.map.update import _descriptor
    rng = np.random.default_rng(3)
    ds = rng.normal(size=(6, 32)) * np.array([[0.1], [5.0], [1.0], [30.0], [2.0], [0.5]])
    ref, mine, cnt = io.Descriptor().add(ds[0]), _descriptor(None, 0, ds[0], 1), 1
    assert mine.tobytes() == ref.value.tobytes()
    plain = ds[0] / np.linalg.norm(ds[0])                   # what a running mean without line 489 would hold
    for d in ds[1:4]:
        ref.add(d)
        mine, plain = _descriptor(mine, cnt, d, 1), plain * cnt / (cnt + 1) + d / np.linalg.norm(d) / (cnt + 1)
        cnt += 1
        assert mine.tobytes() == ref.value.tobytes() and cnt == ref.cnt
        assert abs(np.linalg.norm(mine) - 1.0) <= 4 * io.EPS and np.linalg.norm(plain) < 0.9
        cos = float(mine @ plain / np.linalg.norm(plain))
    assert cos < 1.0 - 1e-6, "after several updates the renormalised mean differs from the plain one in direction"
    other = io.Descriptor().add(ds[4]).add(ds[5])           # a merge: the absorbed segment's descriptor with its count
    ref.add(other.value, other.cnt)
    mine = _descriptor(mine, cnt, other.value, other.cnt)
    assert mine.tobytes() == ref.value.tobytes() and ref.cnt == 6 and abs(np.linalg.norm(mine) - 1.0) <= 4 * io.EPS
