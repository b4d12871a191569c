"""The loop-closure entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes mirror,
and the two new structs laid out as the C compiler lays them out (the way tests/test_abi.py checks roman_params_t)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import lc_record_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_lc_tail_dev", "roman_align_lc_batch_dev", "roman_align_lc_batch")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and fn.argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    for s in ENTRY_POINTS:
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
    # argument counts of the header's prototypes
    assert len(lib.roman_lc_tail_dev.argtypes) == 15 and len(lib.roman_align_lc_batch_dev.argtypes) == 28 and len(lib.roman_align_lc_batch.argtypes) == 31
    src = open(HEADER).read()
    for s, n in zip(ENTRY_POINTS, (15, 28, 31)):
        proto = src[src.index(f"ROMAN_API int {s}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s


def test_lc_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    fp = [f for f, _ in _abi.RomanLcParams._fields_]; fr = [f for f, _ in _abi.RomanLcRecord._fields_]
    body = "\n".join(f'printf("p.{f} %zu\\n", offsetof(roman_lc_params_t, {f}));' for f in fp)
    body += "\n" + "\n".join(f'printf("r.{f} %zu\\n", offsetof(roman_lc_record_t, {f}));' for f in fr)
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof_p %zu\\nsizeof_r %zu\\n", sizeof(roman_lc_params_t), sizeof(roman_lc_record_t));\n{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof_p"]) == C.sizeof(_abi.RomanLcParams) == _abi.LC_PARAMS_NBYTES
    assert int(out["sizeof_r"]) == C.sizeof(_abi.RomanLcRecord) == _abi.LC_RECORD_NBYTES == lc_record_dtype().itemsize
    for f in fp:
        assert int(out[f"p.{f}"]) == getattr(_abi.RomanLcParams, f).offset, f
    dt = lc_record_dtype()
    for f in fr:
        assert int(out[f"r.{f}"]) == getattr(_abi.RomanLcRecord, f).offset == dt.fields[f][1], f


def test_flag_values_match_the_header():
    src = open(HEADER).read()
    for name in ("ACCEPTED", "FAILED_INSUFFICIENT", "FAILED_TILT", "FAILED_UPSIDE_DOWN", "SKIPPED", "INTERNAL"):
        line = next(l for l in src.splitlines() if l.startswith(f"#define ROMAN_LC_{name} "))
        assert int(line.split()[2]) == getattr(_abi, f"ROMAN_LC_{name}")


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    lp = _abi.RomanLcParams(); lp.dim = 3
    n = np.zeros(1, np.int32)
    assert lib.roman_lc_tail_dev(None, C.byref(lp), 0, None, None, None, None, None, None, None, None, None, None, None, C.c_void_p(n.ctypes.data)) != 0
