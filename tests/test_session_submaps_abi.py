"""roman_session_submaps_dev / roman_session_submaps at the C-ABI boundary: exported, declared with the signatures
of include/roman_hip.h, and every refusal answered with its error code before anything touches a device (the offset tables and the
parameter block are judged on host memory; the pattern of tests/test_session_abi.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import submap_desc_dtype

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_session_submaps_dev", "roman_session_submaps")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == 17, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        args = [a.strip() for a in proto[proto.index("(") + 1:].split(",")]
        assert len(args) == 17, s
        assert [k for k, a in enumerate(args) if a.startswith("int32_t ")] == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32] == [2, 3, 15], s
        assert args[4].startswith("const int64_t* seg_off") and args[8].startswith("const int32_t* sub_off") and args[9].startswith("const roman_submap_desc_t*")
    at = src.index("ROMAN_API int roman_session_submaps_dev(")
    assert "[REF roman/map/map.py:297-346]" in src[max(0, at - 4000):at] and "§4.19" in src[max(0, at - 4000):at]
    kern = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    for k in ("k_submap_points", "k_submap_select", "k_submap_gather", "k_submap_desc"):
        assert f" {k}(" in kern, k


class Args:
    """A well-formed call over host memory (never dereferenced as device memory: every case below is refused, or empty)."""

    def __init__(self, n=(5, 0, 7), s=(2, 3, 0), F=6, cap=4, alloc=True):
        self.P = _abi.RomanSubmapParams(3, cap, cap, 0, 1, 0, 15.0)
        self.F, self.desc_dim = F, 2
        self.seg_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        self.sub_off = np.concatenate([[0], np.cumsum(s)]).astype(np.int32)
        N, S = (int(self.seg_off[-1]), int(self.sub_off[-1])) if alloc else (1, 1)
        self.a = dict(feats=np.zeros((N, F)), times=np.zeros((N, 2)), ids=np.zeros(N, np.int64), descs=np.zeros(S, dtype=submap_desc_dtype()),
                      pool=np.zeros((S * cap, F)), count=np.zeros(S, np.int32), src=np.zeros(S * cap, np.int32), ids_out=np.zeros(S * cap, np.int64),
                      status=np.zeros(S, np.int32), desc_out=np.zeros((S, 2)))
        self.R = len(n)

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a = self.a
        fn = lib.roman_session_submaps if host else lib.roman_session_submaps_dev
        return fn(ctx, None if self.P is None else C.byref(self.P), self.R, self.F, p(self.seg_off), p(a["feats"]), p(a["times"]), p(a["ids"]), p(self.sub_off),
                  p(a["descs"]), p(a["pool"]), p(a["count"]), p(a["src"]), p(a["ids_out"]), p(a["status"]), self.desc_dim, p(a["desc_out"]))


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(edit, host):
        a = Args(); edit(a)
        return a.call(lib, host, h)

    def set_(name, value):
        return lambda a: a.a.__setitem__(name, value)

    def attr(name, value):
        return lambda a: setattr(a, name, value)
    for host in (False, True):
        # the session's own
        assert code(attr("R", -1), host) == E.ROMAN_E_INVALID
        assert code(attr("seg_off", None), host) == E.ROMAN_E_INVALID and code(attr("sub_off", None), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.seg_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID and b"must be 0" in lib.roman_last_error(h)
        assert code(lambda a: a.sub_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID and b"must be 0" in lib.roman_last_error(h)
        assert code(lambda a: a.seg_off.__setitem__(2, 3), host) == E.ROMAN_E_INVALID and b"seg_off decreases" in lib.roman_last_error(h)
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID and b"sub_off decreases" in lib.roman_last_error(h)
        assert Args(s=(1 << 20, 1 << 20), n=(1, 1), cap=1 << 10, alloc=False).call(lib, host, h) == E.ROMAN_E_TOO_LARGE      # 2^31 rows: beyond int32
        assert Args(n=(1 << 32, 1), s=(1, 1), alloc=False).call(lib, host, h) == E.ROMAN_E_TOO_LARGE                      # a map beyond int32 rows
        # those of roman_submaps_dev
        assert code(attr("P", None), host) == E.ROMAN_E_INVALID
        for field, bad in (("point_dim", 4), ("cap", 0), ("max_size", 3), ("reserved0", 1), ("radius", float("nan"))):
            assert code(lambda a: setattr(a.P, field, bad), host) == E.ROMAN_E_INVALID, field
        assert code(attr("F", 2), host) == E.ROMAN_E_INVALID
        assert code(attr("desc_dim", 4), host) == E.ROMAN_E_INVALID and code(attr("desc_dim", -1), host) == E.ROMAN_E_INVALID
        assert code(attr("desc_dim", 0), host) == E.ROMAN_E_INVALID                  # desc_out given with desc_dim 0
        assert code(set_("ids", None), host) == E.ROMAN_E_INVALID                    # ids_out without seg_ids
        for name in ("descs", "count", "src", "status", "feats", "times"):
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name
        if not host:                                                                 # (the host form needs no pool)
            assert code(set_("pool", None), host) == E.ROMAN_E_INVALID


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code, a well-formed one
    with ROMAN_E_INVALID for the context, and a call without submaps is empty whatever the context."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        assert Args().call(lib, host) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
        assert Args(n=(), s=()).call(lib, host) == _abi.ROMAN_E_INVALID               # R == 0: legal, and still no context
        assert b"ctx is NULL" in lib.roman_last_error(None)
