"""The batched multi-solution entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes
mirror, and roman_mno_solution_t laid out as the C compiler lays it out (the pattern of tests/test_lc_abi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import mno_solution_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_mno_batch_dev", "roman_mno_batch")
ARG_COUNTS = (16, 17)


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and fn.argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, n in zip(ENTRY_POINTS, ARG_COUNTS):
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        assert len(getattr(lib, s).argtypes) == n, s
        proto = src[src.index(f"ROMAN_API int {s}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        at = src.index(f"ROMAN_API int {s}(")
        assert "[REF roman/align/object_registration.py:57-86]" in src[max(0, at - 6000):at], s    # the comment above cites what it replaces


def test_solution_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.RomanMnoSolution._fields_]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(roman_mno_solution_t, {f}));' for f in fields)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof %zu\\nmaxk %d\\nmaxa %d\\n", sizeof(roman_mno_solution_t), ROMAN_MNO_MAX_SOLUTIONS, ROMAN_MNO_MAX_ASSOC);\n{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = mno_solution_dtype()
    assert int(out["sizeof"]) == C.sizeof(_abi.RomanMnoSolution) == _abi.MNO_SOLUTION_NBYTES == dt.itemsize
    for f in fields:
        assert int(out[f]) == getattr(_abi.RomanMnoSolution, f).offset == dt.fields[f][1], f
    assert int(out["maxk"]) == _abi.ROMAN_MNO_MAX_SOLUTIONS and int(out["maxa"]) == _abi.ROMAN_MNO_MAX_ASSOC


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    P = _abi.RomanParams.default()
    n = np.zeros(1, np.int32)
    v = C.c_void_p(n.ctypes.data)
    assert lib.roman_mno_batch_dev(None, C.byref(P), 0, None, None, None, None, None, 3, None, None, 2, 1, v, v, None) != 0
    assert lib.roman_mno_batch(None, C.byref(P), 0, None, 0, None, None, None, None, 3, None, None, 2, 1, v, v, None) != 0
