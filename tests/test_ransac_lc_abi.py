"""The RANSAC loop-closure entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes
mirror with the signatures of the header, their comments citing what they replace (the pattern of tests/test_ransac_abi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = {"roman_ransac_lc_batch_dev": 26, "roman_ransac_lc_batch": 29}
REFS = ("[REF roman/align/ransac_reg.py:16-53]", "[REF roman/align/submap_align.py:160-200]", "[REF roman/align/results.py:156-198]")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, n in ENTRY_POINTS.items():
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == n, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        above = src[max(0, at - 700):at]                        # the comment directly above the prototype
        for ref in REFS:
            assert ref in above, (s, ref)
    # the two in the RANSAC section, behind the packed calls
    assert src.index("roman_ransac_batch(") < src.index("roman_ransac_lc_batch_dev(") < src.index("submaps from a whole map")


def test_ctypes_signatures_match_the_header():
    """Argument by argument: pointers are void pointers (or the struct's pointer type), int32_t / int64_t scalars as in C."""
    lib = _abi.load_library()
    src = open(HEADER).read()
    P = C.POINTER
    kind = {"roman_ctx_t*": C.c_void_p, "const roman_ransac_params_t*": P(_abi.RomanRansacParams), "const roman_lc_params_t*": P(_abi.RomanLcParams),
            "int32_t": C.c_int32, "int64_t": C.c_int64}
    for s in ENTRY_POINTS:
        at = src.index(f"ROMAN_API int {s}(") + len(f"ROMAN_API int {s}(")
        proto = src[at:src.index(");", at)]
        while "/*" in proto:
            proto = proto[:proto.index("/*")] + proto[proto.index("*/") + 2:]
        want = []
        for arg in proto.split(","):
            t = " ".join(arg.split()[:-1])
            want.append(kind.get(t, C.c_void_p if t.endswith("*") else None))
        assert None not in want, (s, proto)
        assert list(getattr(lib, s).argtypes) == want, s


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    R = _abi.RomanRansacParams(100, 10, 0.95, 0.5, 0.999, 0)
    L = _abi.RomanLcParams(3, 0, 0, 4, -1.0)
    n = np.zeros(64, np.int32)
    v = C.c_void_p(n.ctypes.data)
    assert lib.roman_ransac_lc_batch_dev(None, C.byref(R), 0, None, 3, None, None, None, None, 1, v, v, None, v, v, v,
                                         C.byref(L), None, None, None, None, None, None, v, v, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_ransac_lc_batch(None, C.byref(R), 0, None, 0, 3, None, None, None, None, 1, v, v, None, v, v, v,
                                     C.byref(L), None, None, None, 0, None, None, 0, None, v, v, v) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)
