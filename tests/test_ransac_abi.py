"""The batched RANSAC entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes mirror,
and the two new structs laid out as the C compiler lays them out (the pattern of tests/test_mno_abi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import ransac_record_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_ransac_batch_dev", "roman_ransac_batch")
ARG_COUNTS = (12, 13)


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, n in zip(ENTRY_POINTS, ARG_COUNTS):
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == n, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        assert "[REF roman/align/ransac_reg.py:16-53]" in src[max(0, at - 3000):at], s       # the comment above cites what it replaces
        assert "DEVIATION" in src[max(0, src.index("typedef struct roman_ransac_params") - 4000):at]


def test_struct_layouts_match_c(tmp_path):
    fp = [f for f, _ in _abi.RomanRansacParams._fields_]
    fr = [f for f, _ in _abi.RomanRansacRecord._fields_]
    assert fp == ["max_iteration", "round", "edge_len", "max_dist", "confidence", "seed"]
    assert fr == ["n_assoc", "status", "n_hyp", "n_scored", "best_hyp", "best_count", "best_sse", "T"]
    body = "\n".join(f'printf("p.{f} %zu\\n", offsetof(roman_ransac_params_t, {f}));' for f in fp)
    body += "\n" + "\n".join(f'printf("r.{f} %zu\\n", offsetof(roman_ransac_record_t, {f}));' for f in fr)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof_p %zu\\nsizeof_r %zu\\nmaxn %d\\n", sizeof(roman_ransac_params_t), sizeof(roman_ransac_record_t), ROMAN_RANSAC_MAX_OBJECTS);\n'
                    f'{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = ransac_record_dtype()
    assert int(out["sizeof_p"]) == C.sizeof(_abi.RomanRansacParams)
    assert int(out["sizeof_r"]) == C.sizeof(_abi.RomanRansacRecord) == _abi.RANSAC_RECORD_NBYTES == dt.itemsize
    for f in fp:
        assert int(out[f"p.{f}"]) == getattr(_abi.RomanRansacParams, f).offset, f
    for f in fr:
        assert int(out[f"r.{f}"]) == getattr(_abi.RomanRansacRecord, f).offset == dt.fields[f][1], f
    assert int(out["maxn"]) == _abi.ROMAN_RANSAC_MAX_OBJECTS == 1024


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    P = _abi.RomanRansacParams(100, 10, 0.95, 0.5, 0.999, 0)
    n = np.zeros(1, np.int32)
    v = C.c_void_p(n.ctypes.data)
    assert lib.roman_ransac_batch_dev(None, C.byref(P), 0, None, None, None, None, None, 1, v, v, None) != 0
    assert lib.roman_ransac_batch(None, C.byref(P), 0, None, 0, None, None, None, None, 1, v, v, None) != 0
