"""roman_session_boxes* and roman_session_gate_aabb* at the C-ABI boundary: exported, declared with the signatures
of include/roman_hip.h, and every refusal answered with its error code before anything touches a device — in the style of
tests/test_session_abi.py, whose argument block this one extends."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from test_session_abi import Args

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
N_ARGS = {"roman_session_boxes_dev": 8, "roman_session_boxes": 8, "roman_session_gate_aabb_dev": 29, "roman_session_gate_aabb": 25}


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
        assert ints == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32], s
    at = src.index("ROMAN_API int roman_session_boxes_dev(")
    assert "[REF roman/map/map.py:133-139]" in src[at - 3000:at] and "[REF roman/utils.py:160-169]" in src[at - 3000:at]
    at = src.index("ROMAN_API int roman_session_gate_aabb_dev(")
    assert "[REF roman/align/submap_align.py:101-103]" in src[at - 3000:at] and "[REF roman/utils.py:167-169]" in src[at - 3000:at]
    # the radius-mode entry still refuses a missing radius, and now names the entry that serves it
    hip = open(os.path.join(ROOT, "roman_amd", "csrc", "roman_hip.hip")).read()
    assert "roman_session_gate_aabb*" in hip and "the session gate serves the radius mode only" not in hip


p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)


def check_boxes_error_codes(lib, h):
    """Every refusal of roman_session_boxes*, on the context `h` (None: the arguments are judged first, then the context)."""
    E = _abi
    S, F = 3, 4
    a = dict(pool=np.zeros((12, F)), row0=np.array([0, 4, 8], np.int64), count=np.array([4, 0, 4], np.int32), T=np.zeros((S, 16)), box=np.full((S, 6), 7.0))
    names = ("pool", "row0", "count", "T", "box")
    for fn in (lib.roman_session_boxes_dev, lib.roman_session_boxes):
        call = lambda S_, F_, **edit: fn(h, S_, F_, *[p({**a, **edit}[k]) for k in names])
        assert call(-1, F) == E.ROMAN_E_INVALID and b"S < 0" in lib.roman_last_error(h)
        assert call(S, 2) == E.ROMAN_E_INVALID and b"x y z" in lib.roman_last_error(h)
        for k in names:
            assert call(S, F, **{k: None}) == E.ROMAN_E_INVALID and b"NULL" in lib.roman_last_error(h), k
        if h is None:                                        # well-formed: only the context is missing
            assert call(S, F) == E.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(h)
    bad = lambda **edit: lib.roman_session_boxes(h, S, F, *[p({**a, **edit}[k]) for k in names])
    assert bad(row0=np.array([0, -1, 8], np.int64)) == E.ROMAN_E_INVALID and b"negative" in lib.roman_last_error(h)
    assert bad(count=np.array([4, 0, -2], np.int32)) == E.ROMAN_E_INVALID and b"negative" in lib.roman_last_error(h)
    assert np.all(a["box"] == 7.0)


def test_session_boxes_error_codes_without_a_device():
    check_boxes_error_codes(_abi.load_library(), None)


class AabbArgs(Args):
    """tests/test_session_abi.Args plus the boxes and the nullable sim_in of the AABB entries."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.P.radius = float("nan")                         # (not read: any value is legal)
        self.a["box"] = np.zeros((self.a["pos"].shape[0], 6)); self.a["sim_in"] = None

    def call(self, lib, host, ctx=None):
        a, R, nb = self.a, len(self.sub_off) - 1, len(self.blocks)
        outs = [p(a[k]) for k in ("dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off", "box", "sim_in")]
        ins = [p(a[k]) for k in ("pos", "pos_gt", "has_gt", "T_w", "time", "desc")]
        if host:
            return lib.roman_session_gate_aabb(ctx, C.byref(self.P), R, p(self.sub_off), *ins, nb, p(self.blocks), p(self.pair_off), p(self.tile_off), *outs)
        return lib.roman_session_gate_aabb_dev(ctx, C.byref(self.P), R, p(self.sub_off), p(self.sub_off), *ins, nb, p(self.blocks), p(self.blocks),
                                               p(self.pair_off), p(self.pair_off), p(self.tile_off), p(self.tile_off), *outs)


def check_gate_error_codes(lib, h):
    """roman_session_gate_dev's refusals without those of the radius, plus the box and the rules of sim_in, on the context `h`; with
    h None a well-formed call (a NaN radius included) is refused for its NULL context only."""
    E = _abi

    def code(edit, host):
        a = AabbArgs(); edit(a)
        return a.call(lib, host, h)
    set_ = lambda name, value: (lambda a: a.a.__setitem__(name, value))
    for host in (False, True):
        for name in ("pos", "T_w", "desc", "time", "box", "dist", "flags", "yaw", "sim", "T_ij", "pairs", "T_ref", "enable", "todo_off"):
            assert code(set_(name, None), host) == E.ROMAN_E_INVALID, name
        assert code(set_("box", None), host) == E.ROMAN_E_INVALID and b"box is NULL" in lib.roman_last_error(h)
        assert code(lambda a: a.blocks.__setitem__((1, 1), 2), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.blocks.__setitem__((0, 0), -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.sub_off.__setitem__(1, 6), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.blocks.__setitem__((0, 3), 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "reserved1", 1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: setattr(a.P, "desc_dim", -1), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.pair_off.__setitem__(1, 8), host) == E.ROMAN_E_INVALID
        assert code(lambda a: a.tile_off.__setitem__(2, 5), host) == E.ROMAN_E_INVALID
        assert code(set_("pos_gt", np.zeros((5, 3))), host) == E.ROMAN_E_INVALID
        assert AabbArgs(counts=(12000, 12000), blocks=((0, 1, 0),), alloc=False).call(lib, host, h) == E.ROMAN_E_TOO_LARGE
        assert AabbArgs(counts=(2, 2), blocks=((0, 1, 0), (0, 1, 0))).call(lib, host, h) == E.ROMAN_E_INVALID
        assert b"twice" in lib.roman_last_error(h)
        # sim_in: desc_dim must be 0; then desc and sim may be NULL
        assert code(set_("sim_in", np.zeros(15)), host) == E.ROMAN_E_INVALID and b"desc_dim" in lib.roman_last_error(h)

        def given(a):
            a.P.desc_dim = 0; a.a.update(sim_in=np.zeros(15), desc=None, sim=None)
        for radius in (float("nan"), -1.0, 5.0) if h is None else ():             # the radius is not read: no INVALID for NaN, no UNSUPPORTED for "none"
            for edit in (lambda a: None, given):
                a = AabbArgs(); a.P.radius = radius; edit(a)
                assert a.call(lib, host) == E.ROMAN_E_INVALID and b"ctx is NULL" in lib.roman_last_error(h)


def test_session_gate_aabb_error_codes_without_a_device():
    check_gate_error_codes(_abi.load_library(), None)
