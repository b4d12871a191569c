"""The C-ABI boundary of roman_shared_reduce_dev (include/roman_hip.h) without a GPU: the symbol is exported
and declared with the stated prototype, a NULL context is refused before anything touches a device, and Context.shared_reduce_dev
hands the arguments over in the header's order (through tests/_recording_lib.py behind roman_amd._abi)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from _recording_lib import RecordingLib, _arr
from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import Context

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
NAME = "roman_shared_reduce_dev"
PROTOTYPE = ("roman_ctx_t* ctx, int32_t B, int32_t F, double* feats, int64_t region_row0, const int64_t* ids, const int64_t* off1, "
             "const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t* keep, int32_t* kept")


def test_symbol_exported_and_declared_with_the_stated_prototype():
    lib = _abi.load_library()
    assert NAME in _abi.EXPORTED_SYMBOLS and NAME in lib._roman_symbols
    fn = getattr(lib, NAME)
    vp = C.c_void_p
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    assert f" T {NAME}" in out, f"{NAME} is not an exported text symbol of the built library"
    src = open(HEADER).read()
    at = src.index(f"ROMAN_API int {NAME}(")
    proto = src[at + len(f"ROMAN_API int {NAME}("):]
    proto = re.sub(r"\s+", " ", proto[:proto.index(");")]).strip()
    assert proto == PROTOTYPE
    comment = src[src.rindex("/*", 0, at):at]
    assert "[REF roman/align/submap_align.py:108-115]" in comment and "8 * F * sum (n1 + n2)" in comment
    assert "reads the\n * pool as given" in comment or "pool as given" in comment


def test_null_context_is_refused_without_a_device():
    lib = _abi.load_library()
    assert getattr(lib, NAME)(None, 1, 4, None, 0, None, None, None, None, None, None, None) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)


class Recorder(RecordingLib):
    def __init__(self):
        super().__init__(None)
        self.args = None

    def roman_shared_reduce_dev(self, *a):
        self._log(NAME); self.args = a
        B = a[1]                                                   # the host arrays live as long as the call: decode them now
        self.host = [_arr(a[6], B, np.int64), _arr(a[7], B, np.int32), _arr(a[8], B, np.int64), _arr(a[9], B, np.int32)]
        return 0


def test_the_binding_passes_the_arguments_in_the_headers_order(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_abi, "_LIB", rec)
    ctx = Context(0)
    off1 = np.array([0, 5], dtype=np.int32); n1 = np.array([5, 3], dtype=np.int64)          # wrong dtypes on purpose: the binding converts
    off2 = [5, 8]; n2 = [3, 4]
    ctx.shared_reduce_dev(2, 7, 0x1000, 12, 0x2000, off1, n1, off2, n2, 0x3000, 0x4000)
    assert rec.calls[-1] == NAME and len(rec.args) == 12
    h, B, F, feats, row0, ids, o1, m1, o2, m2, keep, kept = rec.args
    assert h.value == 0x1234 and (B, F, row0) == (2, 7, 12)
    assert [x.value for x in (feats, ids, keep, kept)] == [0x1000, 0x2000, 0x3000, 0x4000]
    assert [x.tolist() for x in rec.host] == [[0, 5], [5, 3], [5, 8], [3, 4]]
    ctx.shared_reduce_dev(0, 1, None, 0, None, np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32), None, None)
    assert rec.args[3] is None and rec.args[5] is None and rec.args[10] is None and rec.args[11] is None
    ctx.close()
