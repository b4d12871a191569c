"""roman_session_gate_list_dev / roman_session_gate_list at the C-ABI boundary: exported, declared with the
signatures of include/roman_hip.h, and every refusal answered with its own error code before anything touches a device — the
tables and the list are validated on their host copies, with a NULL context too."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import grid_gate_params, session_pair_list, session_tables

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
N_ARGS = {"roman_session_gate_list_dev": 30, "roman_session_gate_list": 26}


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
        ints = [k for k, a in enumerate(proto[proto.index("(") + 1:].split(",")) if a.strip().startswith("int32_t ")]
        assert ints == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32], s          # R, nb and L sit where ctypes passes integers
    at = src.index("ROMAN_API int roman_session_gate_list_dev(")
    assert "DESIGN.md §4.20" in src[max(0, at - 4000):at]


def test_pair_list_helper():
    """session_pair_list: the pairs with a touched side, per block row-major, blocks in list order; nothing else."""
    touched = [np.array([0, 0, 1], bool), None, np.array([1, 0], bool)]
    lst = session_pair_list((3, 0, 2), [(0, 0, 1), (0, 2, 0), (1, 2, 0), (2, 2, 1)], touched)
    want = [(0, 0, 2), (0, 1, 2), (0, 2, 0), (0, 2, 1), (0, 2, 2), (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 2, 1), (3, 0, 0), (3, 0, 1), (3, 1, 0)]
    assert lst.dtype == np.int32 and lst.tolist() == [list(x) for x in want]
    assert session_pair_list((3, 0, 2), [(0, 2, 0)], [None, None, None]).shape == (0, 3)


class Args:
    """A well-formed call over host memory (never dereferenced as device memory: every case below is refused, or empty)."""

    def __init__(self, counts=(3, 2), blocks=((0, 0, 1), (0, 1, 0)), lst=((0, 0, 1), (0, 2, 2), (1, 1, 0), (1, 1, 1)), L=None):
        self.P = grid_gate_params(5.0, desc_dim=4)
        self.sub_off, self.blocks, self.pair_off, _ = session_tables(counts, blocks)
        self.list = np.array(lst, dtype=np.int32).reshape(-1, 3)
        self.L = len(self.list) if L is None else L
        S, B, n, nb = int(self.sub_off[-1]), int(self.pair_off[-1]), max(len(self.list), 1), len(blocks)
        f = lambda *s: np.zeros(s)
        self.a = dict(pos=f(S, 3), pos_gt=None, has_gt=None, T_w=f(S, 16), time=f(S), desc=f(S, 4), box=None, sim_in=None, dist=f(n),
                      flags=np.zeros(n, np.int32), yaw=f(n), sim=f(n), T_ij=f(n, 16), pairs=np.zeros((n, 2), np.int32), T_ref=f(n, 16),
                      enable=np.zeros(n, np.int32), todo_off=np.full(nb + 1, -7, np.int32))
        self.B = B

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a, R, nb = self.a, len(self.sub_off) - 1, len(self.blocks)
        outs = [p(a[k]) for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off")]
        ins = [p(a[k]) for k in ("pos", "pos_gt", "has_gt", "T_w", "time", "desc")]
        lst = None if self.list is None else p(self.list)
        if host:
            return lib.roman_session_gate_list(ctx, C.byref(self.P), R, p(self.sub_off), *ins, nb, p(self.blocks), p(self.pair_off), self.L, lst,
                                               p(a["box"]), p(a["sim_in"]), *outs)
        return lib.roman_session_gate_list_dev(ctx, C.byref(self.P), R, p(self.sub_off), p(self.sub_off), *ins, nb, p(self.blocks), p(self.blocks),
                                               p(self.pair_off), p(self.pair_off), self.L, lst, lst, p(a["box"]), p(a["sim_in"]), *outs)


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(edit, host, **kw):
        a = Args(**kw); edit(a)
        return a.call(lib, host, h)

    def set_(name, value):
        return lambda a: a.a.__setitem__(name, value)

    def entry(l, value):
        return lambda a: a.list.__setitem__(l, value)
    for host in (False, True):
        # the tables: roman_session_gate_dev's refusals
        assert code(lambda a: a.blocks.__setitem__((1, 1), 2), host) == E.ROMAN_E_INVALID            # r outside [0, R)
        assert code(lambda a: a.blocks.__setitem__((0, 0), -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID                # sub_off decreases
        assert code(lambda a: a.sub_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.blocks.__setitem__((0, 3), 1), host) == E.ROMAN_E_INVALID            # a reserved word
        assert code(lambda a: a.pair_off.__setitem__(1, 8), host) == E.ROMAN_E_INVALID               # the prefix disagrees
        assert code(lambda a: None, host, counts=(2, 2), blocks=((0, 1, 0), (0, 1, 0)), lst=((0, 0, 0),)) == E.ROMAN_E_INVALID
        assert b"twice" in lib.roman_last_error(h)
        assert code(lambda a: None, host, counts=(12000, 12000), blocks=((0, 1, 0),), lst=((0, 0, 0),)) == E.ROMAN_E_TOO_LARGE    # the tables' own bound
        # the tables are judged in front of the list: a call wrong in both ways answers for its tables
        assert code(lambda a: (a.blocks.__setitem__((0, 3), 1), a.list.__setitem__(0, (5, 0, 0))), host) == E.ROMAN_E_INVALID
        assert b"reserved" in lib.roman_last_error(h)
        # gparams
        assert code(lambda a: setattr(a.P, "reserved1", 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "radius", float("nan")), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "desc_dim", -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "radius", -1.0), host) == E.ROMAN_E_UNSUPPORTED
        assert code(set_("sim_in", np.zeros(15)), host) == E.ROMAN_E_INVALID                         # the similarity is given: desc_dim must be 0
        assert b"desc_dim" in lib.roman_last_error(h)
        # the list
        assert code(lambda a: setattr(a, "L", -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a, "list", None), host) == E.ROMAN_E_INVALID                   # NULL with L > 0
        assert code(entry(3, (2, 0, 0)), host) == E.ROMAN_E_INVALID                                  # b outside [0, nb)
        assert code(entry(0, (-1, 0, 0)), host) == E.ROMAN_E_INVALID
        assert code(entry(1, (0, 3, 0)), host) == E.ROMAN_E_INVALID                                  # i outside the block's rows
        assert code(entry(3, (1, 1, 2)), host) == E.ROMAN_E_INVALID                                  # j outside its columns
        assert code(entry(0, (0, 0, -1)), host) == E.ROMAN_E_INVALID
        assert b"outside" in lib.roman_last_error(h)
        assert code(entry(1, (0, 0, 1)), host) == E.ROMAN_E_INVALID                                  # a pair twice
        assert b"ascending" in lib.roman_last_error(h)
        assert code(entry(2, (0, 1, 0)), host) == E.ROMAN_E_INVALID                                  # ... and an earlier pair behind a later one
        assert code(lambda a: setattr(a, "L", 2 ** 27), host) == E.ROMAN_E_TOO_LARGE                  # L * 16 beyond int32: the list is never read
        # what is needed
        for name in ("pos", "T_w", "desc", "time", "dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name
        assert code(set_("pos_gt", np.zeros((5, 3))), host) == E.ROMAN_E_INVALID                     # pos_gt without has_gt


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code, a well-formed one
    — an empty list included — with ROMAN_E_INVALID for the context."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        for kw in (dict(), dict(lst=())):
            assert Args(**kw).call(lib, host) == _abi.ROMAN_E_INVALID
            assert b"ctx is NULL" in lib.roman_last_error(None)
        a = Args()
        a.a["box"] = np.zeros((5, 6)); a.P.radius = float("nan")     # with the boxes the radius is not read
        assert a.call(lib, host) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)
        a = Args()
        a.a["sim_in"] = np.zeros(a.B); a.P.desc_dim = 0; a.a["desc"] = None
        assert a.call(lib, host) == _abi.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)
