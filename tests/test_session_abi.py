"""roman_session_gate_dev / roman_session_gate at the C-ABI boundary: exported, declared with the signatures of
include/roman_hip.h, the parameter block laid out as declared, and every refusal answered with its error code before anything
touches a device (the tables are validated on their host copies)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _session as ss
from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import grid_gate_params, session_tables

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
N_ARGS = {"roman_session_gate_dev": 27, "roman_session_gate": 23}


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
        assert ints == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32], s          # R and nb sit where ctypes passes integers
    at = src.index("ROMAN_API int roman_session_gate_dev(")
    assert "[REF roman/align/submap_align.py:93-149]" in src[max(0, at - 4000):at] and "[REF demo/demo.py:138-161]" in src[max(0, at - 4000):at]


def test_struct_layout_and_tile_width_match_c(tmp_path):
    """The session gate takes roman_grid_gate_params_t as it is; the tile width of tile_off is the kernels' GRID_TJ."""
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    'printf("%zu %zu %zu\\n", sizeof(roman_grid_gate_params_t), offsetof(roman_grid_gate_params_t, single_robot_lc), '
                    'offsetof(roman_grid_gate_params_t, lc_time_thresh));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    size, lc, thresh = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_abi.RomanGridGateParams) == 56
    assert lc == _abi.RomanGridGateParams.single_robot_lc.offset and thresh == _abi.RomanGridGateParams.lc_time_thresh.offset
    kern = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert f"constexpr int GRID_TJ = {_abi.GRID_TJ};" in kern and f"constexpr int SESSION_SCAN = {_abi.SESSION_SCAN};" in kern


class Args:
    """A well-formed call over host memory (never dereferenced as device memory: every case below is refused, or empty)."""

    def __init__(self, counts=(3, 2), blocks=((0, 0, 1), (0, 1, 0)), alloc=True):
        self.P = grid_gate_params(5.0, desc_dim=4)
        self.sub_off, self.blocks, self.pair_off, self.tile_off = session_tables(counts, blocks)
        S, B, nb = int(self.sub_off[-1]), int(self.pair_off[-1]), len(blocks)
        if not alloc:                                        # (a call that is refused for its size: the arrays are never touched)
            S = B = 1
        f = lambda *s: np.zeros(s)
        self.a = dict(pos=f(S, 3), pos_gt=None, has_gt=None, T_w=f(S, 16), time=f(S), desc=f(S, 4), dist=f(B), flags=np.zeros(B, np.int32), yaw=f(B),
                      sim=f(B), T_ij=f(B, 16), pairs=np.zeros((B, 2), np.int32), T_ref=f(B, 16), enable=np.zeros(B, np.int32),
                      todo_off=np.full(nb + 1, -7, np.int32))

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a, R, nb = self.a, len(self.sub_off) - 1, len(self.blocks)
        outs = [p(a[k]) for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off")]
        ins = [p(a[k]) for k in ("pos", "pos_gt", "has_gt", "T_w", "time", "desc")]
        if host:
            return lib.roman_session_gate(ctx, C.byref(self.P), R, p(self.sub_off), *ins, nb, p(self.blocks), p(self.pair_off), p(self.tile_off), *outs)
        return lib.roman_session_gate_dev(ctx, C.byref(self.P), R, p(self.sub_off), p(self.sub_off), *ins, nb, p(self.blocks), p(self.blocks),
                                          p(self.pair_off), p(self.pair_off), p(self.tile_off), p(self.tile_off), *outs)


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(edit, host):
        a = Args(); edit(a)
        return a.call(lib, host, h)

    def set_(name, value):
        return lambda a: a.a.__setitem__(name, value)
    for host in (False, True):
        for name in ("pos", "T_w", "desc", "time", "dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name
        assert code(lambda a: a.blocks.__setitem__((1, 1), 2), host) == E.ROMAN_E_INVALID            # r outside [0, R)
        assert code(lambda a: a.blocks.__setitem__((0, 0), -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID                # sub_off decreases
        assert code(lambda a: a.blocks.__setitem__((0, 3), 1), host) == E.ROMAN_E_INVALID            # a reserved word
        assert code(lambda a: setattr(a.P, "reserved1", 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "radius", float("nan")), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "desc_dim", -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.pair_off.__setitem__(1, 8), host) == E.ROMAN_E_INVALID               # the prefixes disagree
        assert code(lambda a: a.tile_off.__setitem__(2, 5), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "radius", -1.0), host) == E.ROMAN_E_UNSUPPORTED
        assert code(set_("pos_gt", np.zeros((5, 3))), host) == E.ROMAN_E_INVALID                     # pos_gt without has_gt
        assert Args(counts=(12000, 12000), blocks=((0, 1, 0),), alloc=False).call(lib, host, h) == E.ROMAN_E_TOO_LARGE     # 1.44e8 pairs * 16: beyond int32
        assert Args(counts=(2, 2), blocks=((0, 1, 0), (0, 1, 0))).call(lib, host, h) == E.ROMAN_E_INVALID
        assert b"twice" in lib.roman_last_error(h)


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code, a well-formed one
    with ROMAN_E_INVALID for the context."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        assert Args().call(lib, host) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
