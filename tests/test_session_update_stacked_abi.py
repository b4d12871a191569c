"""roman_session_stacked_sim_list* at the C-ABI boundary: exported, declared with the signatures of
include/roman_hip.h, and every refusal answered with its error code before anything touches a device, in the order the header
states: the tables, then what roman_session_stacked_sim_dev refuses about d, the views and its pointers, then the list as
roman_session_gate_list_dev judges it, then sim."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from test_session_stacked_abi import Args as StackedArgs

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
N_ARGS = {"roman_session_stacked_sim_list_dev": 23, "roman_session_stacked_sim_list": 17}


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, n in N_ARGS.items():
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == n, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == n, s
        args = [a.strip() for a in proto[proto.index("(") + 1:].split(",")]
        assert [k for k, a in enumerate(args) if a.startswith("int32_t ")] == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32], s
        assert [k for k, a in enumerate(args) if a.startswith("int64_t ")] == [k for k, t in enumerate(fn.argtypes) if t is C.c_int64], s
    # the whole-block call's arguments up to pair_off (sim moves to the end), then L, the list (twice on the device form) and sim
    for a, b, extra in (("roman_session_stacked_sim_dev", "roman_session_stacked_sim_list_dev", 3), ("roman_session_stacked_sim", "roman_session_stacked_sim_list", 2)):
        fa, fb = getattr(lib, a).argtypes, getattr(lib, b).argtypes
        assert fb[:len(fa) - 1] == fa[:-1] and fb[len(fa) - 1] is C.c_int32 and all(t is C.c_void_p for t in fb[len(fa):]) and len(fb) == len(fa) + extra


class Args(StackedArgs):
    """A well-formed call over host memory (never dereferenced as device memory: every case below is refused, or empty).  The
    default list: the first and the last pair of both blocks (3 x 3 and 3 x 2)."""

    def __init__(self, lst=((0, 0, 0), (0, 2, 2), (1, 0, 0), (1, 2, 1)), **kw):
        super().__init__(**kw)
        self.list = np.array(lst, dtype=np.int32).reshape(-1, 3)
        self.L = len(self.list)
        self.list_on_device = True                           # False: the device form gets a NULL device list beside the host copy

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a, R, nb = self.a, self.R, self.nb
        t = [self.frame_lo, self.frame_n, self.mask_off, self.sub_off]
        if host:
            return lib.roman_session_stacked_sim_list(ctx, self.d, self.Nf, p(a["desc"]), p(a["mask"]), self.mask_words, R, *[p(x) for x in t], nb, p(self.blocks),
                                                      p(self.pair_off), self.L, p(self.list), p(a["sim"]))
        twice = lambda x: (p(x), p(x))
        return lib.roman_session_stacked_sim_list_dev(ctx, self.d, self.Nf, p(a["desc"]), p(a["mask"]), R, *[q for x in t for q in twice(x)], nb, *twice(self.blocks),
                                                      *twice(self.pair_off), self.L, p(self.list) if self.list_on_device else None, p(self.list), p(a["sim"]))


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(*edits, host, **kw):
        a = Args(**kw)
        for edit in edits:
            edit(a)
        return a.call(lib, host, h)

    def said(text):
        return text in lib.roman_last_error(h)
    set_ = lambda name, value: (lambda a: a.a.__setitem__(name, value))
    attr = lambda name, value: (lambda a: setattr(a, name, value))
    item = lambda name, at, value: (lambda a: getattr(a, name).__setitem__(at, value))
    bad_tables, bad_d, bad_view = item("pair_off", 1, 8), attr("d", 0), item("frame_n", 1, -1)
    bad_list, no_sim = item("list", (1, 1), 3), set_("sim", None)
    for host in (False, True):
        # 1. the tables
        for name in ("frame_lo", "frame_n", "mask_off", "sub_off", "blocks", "pair_off"):
            assert code(attr(name, None), host=host) == E.ROMAN_E_INVALID, name
        assert code(attr("Nf", -1), host=host) == E.ROMAN_E_INVALID
        assert code(item("blocks", (1, 1), 2), host=host) == E.ROMAN_E_INVALID               # r outside [0, R)
        assert code(item("sub_off", 1, 6), host=host) == E.ROMAN_E_INVALID                   # sub_off decreases
        assert code(item("sub_off", 0, 1), host=host) == E.ROMAN_E_INVALID
        assert code(item("blocks", (0, 3), 1), host=host) == E.ROMAN_E_INVALID               # a reserved word
        assert code(bad_tables, host=host) == E.ROMAN_E_INVALID and said(b"pair_off")        # the prefix disagrees
        assert code(host=host, counts=(2, 2), blocks=((0, 1, 0), (0, 1, 0)), lst=()) == E.ROMAN_E_INVALID and said(b"twice")
        assert code(host=host, counts=(12000, 12000), blocks=((0, 1, 0),), lst=()) == E.ROMAN_E_TOO_LARGE
        # ... in front of everything else: of d, of the views, of the list, of sim
        assert code(bad_tables, bad_d, bad_view, bad_list, no_sim, host=host) == E.ROMAN_E_INVALID and said(b"pair_off")
        assert code(bad_d, attr("L", -1), host=host, counts=(12000, 12000), blocks=((0, 1, 0),)) == E.ROMAN_E_TOO_LARGE
        # 2. roman_session_stacked_sim_dev's own: d, the frame ranges, mask_off, the pointers it needs
        assert code(bad_d, bad_view, bad_list, no_sim, host=host) == E.ROMAN_E_INVALID and said(b"d=0")
        assert code(attr("Nf", 102), host=host) == E.ROMAN_E_INVALID                         # view 1 ends at frame 103
        assert code(item("frame_lo", 0, -1), host=host) == E.ROMAN_E_INVALID
        assert code(bad_view, bad_list, no_sim, host=host) == E.ROMAN_E_INVALID and said(b"view 1")
        assert code(item("frame_lo", 1, 2**31 - 1), host=host) == E.ROMAN_E_INVALID          # lo + n is added in 64 bits
        assert code(item("mask_off", 1, -1), attr("L", -1), host=host) == E.ROMAN_E_INVALID and said(b"mask_off")
        for name in ("desc", "mask"):
            assert code(set_(name, None), bad_list, no_sim, host=host) == E.ROMAN_E_INVALID and said(b"desc / mask"), name
        # 3. the list, as roman_session_gate_list_dev judges it; sim last
        assert code(attr("L", -1), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"L=-1")
        assert code(attr("list", None), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"list")
        assert code(item("list", (0, 0), -1), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"names block")
        assert code(item("list", (3, 0), 2), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"names block")
        assert code(bad_list, no_sim, host=host) == E.ROMAN_E_INVALID and said(b"lies outside")              # i == n0
        assert code(item("list", (3, 2), 2), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"lies outside")   # j == n1
        assert code(item("list", (0, 1), -1), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"lies outside")
        assert code(item("list", (1, slice(None)), (0, 0, 0)), no_sim, host=host) == E.ROMAN_E_INVALID and said(b"strictly ascending")   # a pair twice
        assert code(no_sim, host=host, lst=((1, 0, 0), (0, 0, 0))) == E.ROMAN_E_INVALID and said(b"strictly ascending")
        assert code(no_sim, host=host) == E.ROMAN_E_INVALID and said(b"sim is NULL")
    # the host copies are judged in front of the device pointers: a NULL device list comes behind every refusal above
    no_dev_list = attr("list_on_device", False)
    assert code(no_dev_list, host=False, counts=(12000, 12000), blocks=((0, 1, 0),)) == E.ROMAN_E_TOO_LARGE
    assert code(no_dev_list, bad_d, host=False) == E.ROMAN_E_INVALID and said(b"d=0")
    assert code(no_dev_list, bad_list, host=False) == E.ROMAN_E_INVALID and said(b"lies outside")
    assert code(no_dev_list, no_sim, host=False) == E.ROMAN_E_INVALID and said(b"sim is NULL")
    assert code(no_dev_list, host=False) == E.ROMAN_E_INVALID and said(b"on the device")
    assert code(no_dev_list, host=False, lst=()) == (E.ROMAN_E_INVALID if h is None else E.ROMAN_OK)         # L == 0 needs no list: as far as the context
    assert h is not None or said(b"ctx is NULL")
    assert code(attr("mask_words", 3 * 2 + 2 * 1 - 1), host=True) == E.ROMAN_E_INVALID       # the host twin copies `mask`: a view may not leave it
    assert code(attr("mask_words", -1), host=True) == E.ROMAN_E_INVALID


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code, a well-formed one —
    an empty list included, with or without sim — with ROMAN_E_INVALID for the context."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        for a, drop_sim in ((Args(), False), (Args(lst=()), False), (Args(lst=()), True)):
            if drop_sim:
                a.a["sim"] = None                            # L == 0 writes nothing: sim may be NULL
            assert a.call(lib, host) == _abi.ROMAN_E_INVALID
            assert b"ctx is NULL" in lib.roman_last_error(None)
        # desc and mask are needed only while a block has submaps and frames on both sides: here robot 1 has submaps and no frame,
        # so with Nf > 0 and L > 0 both may be NULL — the call is well-formed and gets as far as the context
        a = Args(counts=(3, 2), frames=(70, 0), blocks=((0, 1, 0),), lst=((0, 0, 0), (0, 2, 1)))
        a.a["desc"] = a.a["mask"] = None
        assert a.Nf == 70 and a.L == 2
        assert a.call(lib, host) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)
        a = Args(counts=(3, 2), frames=(70, 1), blocks=((0, 1, 0),), lst=((0, 0, 0), (0, 2, 1)))       # one frame: the block is live
        a.a["desc"] = None
        assert a.call(lib, host) == _abi.ROMAN_E_INVALID and b"desc / mask" in lib.roman_last_error(None)
