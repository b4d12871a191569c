"""roman_session_submaps_list_dev / roman_session_submaps_list at the C-ABI boundary: exported, declared with the
signatures of include/roman_hip.h, and every refusal answered with its error code before anything touches a device — the session
tables, the parameter block and the list are judged on host memory (the pattern of tests/test_session_submaps_abi.py, whose
well-formed call this one extends by L, list and changed)."""
import ctypes as C
import os
import subprocess

import numpy as np

import test_session_submaps_abi as base
from conftest import ROOT
from roman_amd import _abi

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_session_submaps_list_dev", "roman_session_submaps_list")


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == 20, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        args = [a.strip() for a in proto[proto.index("(") + 1:].split(",")]
        assert len(args) == 20, s
        assert [k for k, a in enumerate(args) if a.startswith("int32_t ")] == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32] == [2, 3, 15, 17], s
        assert args[4].startswith("const int64_t* seg_off") and args[8].startswith("const int32_t* sub_off") and args[9].startswith("const roman_submap_desc_t*")
        assert args[17] == "int32_t L" and args[18] == "const int32_t* list" and args[19] == "int32_t* changed"
        assert "[REF roman/map/map.py:297-346]" in src[max(0, at - 3500):at] and "§4.21" in src[max(0, at - 6000):at], s
    kern = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    for k in ("k_submap_select", "k_submap_store_list"):
        assert f" {k}(" in kern, k


class Args(base.Args):
    """tests/test_session_submaps_abi.Args plus a list over its five submaps (host memory, never dereferenced as device memory)."""

    def __init__(self, lst=(0, 2, 4), **kw):
        super().__init__(**kw)
        self.lst = None if lst is None else np.array(lst, dtype=np.int32)
        self.L = 0 if lst is None else len(lst)
        self.changed = np.zeros(max(self.L, 1), np.int32)

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a = self.a
        fn = lib.roman_session_submaps_list if host else lib.roman_session_submaps_list_dev
        return fn(ctx, None if self.P is None else C.byref(self.P), self.R, self.F, p(self.seg_off), p(a["feats"]), p(a["times"]), p(a["ids"]), p(self.sub_off),
                  p(a["descs"]), p(a["pool"]), p(a["count"]), p(a["src"]), p(a["ids_out"]), p(a["status"]), self.desc_dim, p(a["desc_out"]),
                  self.L, p(self.lst), p(self.changed))


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
        # the list's own
        assert code(attr("L", -1), host) == E.ROMAN_E_INVALID and b"L < 0" in lib.roman_last_error(h)
        assert code(attr("lst", None), host) == E.ROMAN_E_INVALID and b"list is NULL" in lib.roman_last_error(h)
        for bad in ((0, 2, 5), (-1, 2, 4)):
            assert Args(lst=bad).call(lib, host, h) == E.ROMAN_E_INVALID and b"outside the 5 submaps" in lib.roman_last_error(h), bad
        for bad in ((0, 2, 2), (2, 0, 4)):
            assert Args(lst=bad).call(lib, host, h) == E.ROMAN_E_INVALID and b"not strictly ascending" in lib.roman_last_error(h), bad
        assert Args(lst=(0,), n=(5, 7), s=(0, 0)).call(lib, host, h) == E.ROMAN_E_INVALID                 # no submap at all: every entry is outside
        # the session's own
        assert code(attr("R", -1), host) == E.ROMAN_E_INVALID
        assert code(attr("seg_off", None), host) == E.ROMAN_E_INVALID and code(attr("sub_off", None), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.seg_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID and b"must be 0" in lib.roman_last_error(h)
        assert code(lambda a: a.sub_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID and b"must be 0" in lib.roman_last_error(h)
        assert code(lambda a: a.seg_off.__setitem__(2, 3), host) == E.ROMAN_E_INVALID and b"seg_off decreases" in lib.roman_last_error(h)
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID and b"sub_off decreases" in lib.roman_last_error(h)
        assert Args(s=(1 << 20, 1 << 20), n=(1, 1), cap=1 << 10, alloc=False).call(lib, host, h) == E.ROMAN_E_TOO_LARGE
        assert Args(n=(1 << 32, 1), s=(1, 1), alloc=False, lst=(0,)).call(lib, host, h) == E.ROMAN_E_TOO_LARGE
        # those of roman_submaps_dev
        assert code(attr("P", None), host) == E.ROMAN_E_INVALID
        for field, bad in (("point_dim", 4), ("cap", 0), ("max_size", 3), ("reserved0", 1), ("radius", float("nan"))):
            assert code(lambda a: setattr(a.P, field, bad), host) == E.ROMAN_E_INVALID, field
        assert code(attr("F", 2), host) == E.ROMAN_E_INVALID
        assert code(attr("desc_dim", 4), host) == E.ROMAN_E_INVALID and code(attr("desc_dim", -1), host) == E.ROMAN_E_INVALID
        assert code(attr("desc_dim", 0), host) == E.ROMAN_E_INVALID                  # desc_out given with desc_dim 0
        assert code(set_("ids", None), host) == E.ROMAN_E_INVALID                    # ids_out without seg_ids
        for name in ("descs", "count", "src", "status", "feats", "times", "pool"):   # (the host form needs the pool too: `changed` compares with it)
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code; a well-formed one — an
    empty list, L == 0 with a NULL list, included — passes every check and is stopped by the context alone."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        for ok in (Args(), Args(lst=()), Args(lst=None), Args(lst=(0, 1, 2, 3, 4)), Args(lst=(), n=(), s=())):
            assert ok.call(lib, host) == _abi.ROMAN_E_INVALID
            assert b"ctx is NULL" in lib.roman_last_error(None)
