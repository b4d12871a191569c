"""The hypothesis-tail entry points at the C-ABI boundary, without a GPU: exported by the library, declared in the ctypes mirror
with the header's argument counts, cited, the two structs they exchange laid out as the C compiler lays them out, and the one
refusal that needs no context (the others need a roman_ctx and are tested in tests/test_gpu_mno_lc_tail.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import lc_record_dtype, mno_solution_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_mno_lc_tail_dev", "roman_mno_lc_batch_dev", "roman_mno_lc_batch")
ARG_COUNTS = (17, 29, 32)


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
        proto = src[at:]; proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        above = src[src.rindex(");", 0, at):at]                     # the comment between the previous prototype and this one
        assert "[REF roman/align/object_registration.py:57-86]" in above and "[REF roman/align/results.py:156-198]" in above, s


def test_runtime_wrappers_exist():
    from roman_amd.runtime import Context, LoopClosureResult, MnoLoopClosureResult
    for name in ("mno_lc_tail_dev", "mno_lc_batch_dev", "mno_lc_batch"):
        assert callable(getattr(Context, name))
    assert {"records", "best", "accepted", "accepted_best"} <= set(MnoLoopClosureResult.__dataclass_fields__)
    assert "records" in LoopClosureResult.__dataclass_fields__


def test_exchanged_structs_match_c(tmp_path):
    """roman_mno_solution_t is read and roman_lc_record_t written by lane k at index b * K + k: sizes and offsets as compiled."""
    fs = [f for f, _ in _abi.RomanMnoSolution._fields_]; fr = [f for f, _ in _abi.RomanLcRecord._fields_]
    body = "\n".join(f'printf("s.{f} %zu\\n", offsetof(roman_mno_solution_t, {f}));' for f in fs)
    body += "\n" + "\n".join(f'printf("r.{f} %zu\\n", offsetof(roman_lc_record_t, {f}));' for f in fr)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof_s %zu\\nsizeof_r %zu\\nmaxk %d\\n", sizeof(roman_mno_solution_t), sizeof(roman_lc_record_t), ROMAN_MNO_MAX_SOLUTIONS);\n{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    ds, dr = mno_solution_dtype(), lc_record_dtype()
    assert int(out["sizeof_s"]) == C.sizeof(_abi.RomanMnoSolution) == ds.itemsize
    assert int(out["sizeof_r"]) == C.sizeof(_abi.RomanLcRecord) == dr.itemsize
    assert int(out["maxk"]) == _abi.ROMAN_MNO_MAX_SOLUTIONS == 64       # a problem's hypotheses fit one wave64
    for f in fs:
        assert int(out[f"s.{f}"]) == getattr(_abi.RomanMnoSolution, f).offset == ds.fields[f][1], f
    for f in fr:
        assert int(out[f"r.{f}"]) == getattr(_abi.RomanLcRecord, f).offset == dr.fields[f][1], f


def test_null_context_is_refused_without_a_device():
    """ROMAN_E_INVALID with its text, not a crash: the check runs before anything touches the GPU."""
    lib = _abi.load_library()
    P = _abi.RomanParams.default()
    lp = _abi.RomanLcParams(); lp.dim = 3
    n = np.zeros(4, np.int32)
    v = C.c_void_p(n.ctypes.data)
    assert lib.roman_mno_lc_tail_dev(None, C.byref(lp), 0, 2, None, None, None, None, None, None, None, None, None, None, v, None, v) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)
    assert lib.roman_mno_lc_batch_dev(None, C.byref(P), 0, None, None, None, None, None, 3, None, None, 2, 1, v, v, None,
                                      C.byref(lp), None, None, None, None, None, None, None, None, None, v, None, v) == _abi.ROMAN_E_INVALID
    assert lib.roman_mno_lc_batch(None, C.byref(P), 0, None, 0, None, None, None, None, 3, None, None, 2, 1, v, v, None,
                                  C.byref(lp), None, None, None, 0, None, None, 0, None, None, None, None, v, None, v) == _abi.ROMAN_E_INVALID
