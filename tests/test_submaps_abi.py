"""The submap entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes mirror, and the two
new structs laid out as the C compiler lays them out (the pattern of tests/test_ransac_abi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import submap_desc_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_submaps_dev", "roman_submaps")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == 16, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == 16, s
        assert "[REF roman/map/map.py:297-3" in src[max(0, at - 7000):at], s          # the comment above cites what it replaces


def test_struct_layouts_match_c(tmp_path):
    fp = [f for f, _ in _abi.RomanSubmapParams._fields_]
    fd = [f for f, _ in _abi.RomanSubmapDesc._fields_]
    assert fp == ["point_dim", "max_size", "cap", "prune_by_time", "use_radius", "reserved0", "radius", "reserved"]
    assert fd == ["pos", "T_center_odom", "time", "t_hi", "t_lo"]
    body = "\n".join(f'printf("p.{f} %zu\\n", offsetof(roman_submap_params_t, {f}));' for f in fp)
    body += "\n" + "\n".join(f'printf("d.{f} %zu\\n", offsetof(roman_submap_desc_t, {f}));' for f in fd)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof_p %zu\\nsizeof_d %zu\\n", sizeof(roman_submap_params_t), sizeof(roman_submap_desc_t));\n'
                    f'{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = submap_desc_dtype()
    assert int(out["sizeof_p"]) == C.sizeof(_abi.RomanSubmapParams) == _abi.SUBMAP_PARAMS_NBYTES
    assert int(out["sizeof_d"]) == C.sizeof(_abi.RomanSubmapDesc) == _abi.SUBMAP_DESC_NBYTES == dt.itemsize
    for f in fp:
        assert int(out[f"p.{f}"]) == getattr(_abi.RomanSubmapParams, f).offset, f
    for f in fd:
        assert int(out[f"d.{f}"]) == getattr(_abi.RomanSubmapDesc, f).offset == dt.fields[f][1], f


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    P = _abi.RomanSubmapParams(3, 10, 10, 0, 1, 0, 15.0)
    n = np.zeros(4, np.int64)
    v = C.c_void_p(n.ctypes.data)
    for fn in (lib.roman_submaps_dev, lib.roman_submaps):
        assert fn(None, C.byref(P), 0, 3, None, None, None, 0, None, v, v, v, None, v, 0, None) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)
