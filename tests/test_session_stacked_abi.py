"""roman_session_stacked_sim* and roman_session_gate_sim* at the C-ABI boundary: exported, declared with the
signatures of include/roman_hip.h, the item record laid out as the kernels read it, and every refusal answered with its error code
before anything touches a device (the tables are validated on their host copies)."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import session_tables
from test_session_abi import Args as GateArgs

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
N_ARGS = {"roman_session_stacked_sim_dev": 20, "roman_session_stacked_sim": 15, "roman_session_gate_sim_dev": 28, "roman_session_gate_sim": 24}


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
    # the gate over a given similarity takes the session gate's arguments and one more, at the end
    for a, b in (("roman_session_gate_dev", "roman_session_gate_sim_dev"), ("roman_session_gate", "roman_session_gate_sim")):
        assert getattr(lib, b).argtypes[:-1] == getattr(lib, a).argtypes and getattr(lib, b).argtypes[-1] is C.c_void_p


def test_the_item_record_and_the_band_tile_match_the_kernels():
    kern = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert "struct SsItem { int64_t band_off, tile_off, r_off; int32_t wg_off, block, a0, h; };" in kern
    assert "static_assert(sizeof(SsItem) == 40" in kern and f"constexpr int STACK_TILE = {_abi.STACKED_BAND_MIN};" in kern
    assert "template <bool SIM_IN>\n__global__ void __launch_bounds__(256) k_session_gate(" in kern


class Args:
    """A well-formed call over host memory (never dereferenced as device memory: every case below is refused, or empty)."""

    def __init__(self, counts=(3, 2), frames=(70, 33), blocks=((0, 0, 1), (0, 1, 0)), d=4):
        self.d, self.Nf = d, int(sum(frames))
        self.sub_off, self.blocks, self.pair_off, _ = session_tables(counts, blocks)
        self.frame_lo = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int32)
        self.frame_n = np.array(frames, dtype=np.int32)
        words = [n * ((f + 63) // 64) for n, f in zip(counts, frames)]
        self.mask_off = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.mask_words = int(sum(words))
        self.R, self.nb = len(counts), len(blocks)
        self.a = dict(desc=np.zeros(8), mask=np.zeros(8, np.uint64), sim=np.zeros(8))       # (never read: no call below gets that far)

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a, R, nb = self.a, self.R, self.nb
        t = [self.frame_lo, self.frame_n, self.mask_off, self.sub_off]
        if host:
            return lib.roman_session_stacked_sim(ctx, self.d, self.Nf, p(a["desc"]), p(a["mask"]), self.mask_words, R, *[p(x) for x in t], nb, p(self.blocks),
                                                 p(self.pair_off), p(a["sim"]))
        twice = lambda x: (p(x), p(x))
        return lib.roman_session_stacked_sim_dev(ctx, self.d, self.Nf, p(a["desc"]), p(a["mask"]), R, *[q for x in t for q in twice(x)], nb, *twice(self.blocks),
                                                 *twice(self.pair_off), p(a["sim"]))


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(edit, host, **kw):
        a = Args(**kw); edit(a)
        return a.call(lib, host, h)

    def set_(name, value):
        return lambda a: a.a.__setitem__(name, value)
    for host in (False, True):
        for name in ("desc", "mask", "sim"):
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name
        for name in ("frame_lo", "frame_n", "mask_off", "sub_off", "blocks", "pair_off"):
            assert code(lambda a: setattr(a, name, None), host) == E.ROMAN_E_INVALID, name
        assert code(lambda a: setattr(a, "d", 0), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a, "Nf", -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a, "Nf", 102), host) == E.ROMAN_E_INVALID                      # view 1 ends at frame 103
        assert code(lambda a: a.frame_lo.__setitem__(0, -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.frame_n.__setitem__(1, -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.frame_lo.__setitem__(1, 2**31 - 1), host) == E.ROMAN_E_INVALID       # lo + n is added in 64 bits
        assert code(lambda a: a.mask_off.__setitem__(1, -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.blocks.__setitem__((1, 1), 2), host) == E.ROMAN_E_INVALID            # r outside [0, R)
        assert code(lambda a: a.blocks.__setitem__((0, 0), -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID                # sub_off decreases
        assert code(lambda a: a.sub_off.__setitem__(0, 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.blocks.__setitem__((0, 3), 1), host) == E.ROMAN_E_INVALID            # a reserved word
        assert code(lambda a: a.pair_off.__setitem__(1, 8), host) == E.ROMAN_E_INVALID               # the prefix disagrees
        assert code(lambda a: None, host, counts=(2, 2), blocks=((0, 1, 0), (0, 1, 0))) == E.ROMAN_E_INVALID
        assert b"twice" in lib.roman_last_error(h)
        # the three bounds of the header: pairs, column-maximum workgroups of a round, tiles of a round
        assert code(lambda a: None, host, counts=(12000, 12000), blocks=((0, 1, 0),)) == E.ROMAN_E_TOO_LARGE
        assert code(lambda a: None, host, counts=(11000, 1), frames=(1, 2**31 - 2), blocks=((0, 1, 0),)) == E.ROMAN_E_TOO_LARGE
        assert b"launch width" in lib.roman_last_error(h)
        assert code(lambda a: None, host, counts=(1, 1), frames=(2**29, 2**29), blocks=((0, 1, 0),)) == E.ROMAN_E_TOO_LARGE     # 2^48 tiles
        assert b"tiles" in lib.roman_last_error(h)
    assert code(lambda a: setattr(a, "mask_words", 3 * 2 + 2 * 1 - 1), True) == E.ROMAN_E_INVALID    # the host twin copies `mask`: a view may not leave it
    assert code(lambda a: setattr(a, "mask_words", -1), True) == E.ROMAN_E_INVALID

    # the gate over a given similarity: the session gate's refusals, sim_in in the place of sim, and desc_dim must be 0
    def gate(edit, host, sim_in=True):
        g = GateArgs(); g.P.desc_dim = 0; edit(g)
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a, R, nb = g.a, len(g.sub_off) - 1, len(g.blocks)
        outs = [p(a[k]) for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off")]
        ins = [p(a[k]) for k in ("pos", "pos_gt", "has_gt", "T_w", "time", "desc")]
        given = p(np.zeros(8)) if sim_in else None
        if host:
            return lib.roman_session_gate_sim(h, C.byref(g.P), R, p(g.sub_off), *ins, nb, p(g.blocks), p(g.pair_off), p(g.tile_off), *outs, given)
        return lib.roman_session_gate_sim_dev(h, C.byref(g.P), R, p(g.sub_off), p(g.sub_off), *ins, nb, p(g.blocks), p(g.blocks),
                                              p(g.pair_off), p(g.pair_off), p(g.tile_off), p(g.tile_off), *outs, given)
    for host in (False, True):
        assert gate(lambda g: setattr(g.P, "desc_dim", 4), host) == E.ROMAN_E_INVALID
        assert b"desc_dim must be 0" in lib.roman_last_error(h)
        assert gate(lambda g: None, host, sim_in=False) == E.ROMAN_E_INVALID
        for name in ("pos", "T_w", "time", "dist", "flags", "yaw", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert gate(lambda g: g.a.__setitem__(name, None), host) == E.ROMAN_E_INVALID, name
        assert gate(lambda g: setattr(g.P, "radius", -1.0), host) == E.ROMAN_E_UNSUPPORTED
        assert gate(lambda g: g.tile_off.__setitem__(2, 5), host) == E.ROMAN_E_INVALID
        for name in ("desc", "sim"):                         # not read, not written: may be NULL — the call gets as far as the context
            if h is None:
                assert gate(lambda g: g.a.__setitem__(name, None), host) == E.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(None)


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code, a well-formed one
    with ROMAN_E_INVALID for the context."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    for host in (False, True):
        assert Args().call(lib, host) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
