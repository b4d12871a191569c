"""roman_session_frame_select_list_dev / roman_session_frame_select_list at the C-ABI boundary: exported, declared
with the signatures of include/roman_hip.h, the robot record laid out as the header's, and every refusal answered with its error
code, in the header's order, before anything touches a device — the parameter block, the robots' records and the list are judged on
host memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import frame_select_params, session_frame_robot_dtype, session_frame_robots

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = ("roman_session_frame_select_list_dev", "roman_session_frame_select_list")
NARGS = 19


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s in ENTRY_POINTS:
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == NARGS, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        at = src.index(f"ROMAN_API int {s}(")
        proto = src[at:]
        proto = proto[:proto.index(");")]
        args = [a.strip() for a in proto[proto.index("(") + 1:].split(",")]
        assert len(args) == NARGS, s
        assert [k for k, a in enumerate(args) if a.startswith("int32_t ")] == [k for k, t in enumerate(fn.argtypes) if t is C.c_int32] == [2, 4, 10, 12], s
        assert args[1].startswith("const roman_frame_select_params_t*") and args[3] == "const roman_session_frame_robot_t* robots"
        assert args[12] == "int32_t L" and args[13] == "const int32_t* list" and args[18] == "int32_t* changed"
    at = src.index("ROMAN_API int roman_session_frame_select_list_dev(")
    assert "[REF roman/map/map.py:210-242]" in src[at - 3500:at] and "§4.23" in src[at - 3500:at]


def test_robot_record_matches_the_header():
    src = open(HEADER).read()
    body = src[src.index("typedef struct roman_session_frame_robot {"):src.index("} roman_session_frame_robot_t;")]
    fields = re.findall(r"^\s*(int64_t|int32_t)\s+(\w+)(\[(\d+)\])?;", body, flags=re.M)
    want = [(n, {"int64_t": 8, "int32_t": 4}[t] * int(k or 1)) for t, n, _, k in fields]
    assert [n for n, _ in want] == ["seg0", "mask_off", "n_seg", "sub0", "n_sub", "frame0", "n_frames", "mask_words", "reserved"]
    S, dt = _abi.RomanSessionFrameRobot, session_frame_robot_dtype()
    at = 0
    for name, size in want:
        f = getattr(S, name)
        assert (f.offset, f.size) == (at, size) and dt.fields[name][1] == at, name
        at += size
    assert at == C.sizeof(S) == dt.itemsize == _abi.SESSION_FRAME_ROBOT_NBYTES == 48
    rec = session_frame_robots([5, 0, 7], [2, 0, 3], [65, 10, 0], [4, 1, 0])
    assert rec["seg0"].tolist() == [0, 5, 5] and rec["sub0"].tolist() == [0, 2, 2] and rec["frame0"].tolist() == [0, 65, 75]
    assert rec["mask_off"].tolist() == [0, 8, 8] and rec["mask_words"].tolist() == [4, 1, 0] and not rec["reserved"].any()
    assert session_frame_robots([5], [2], [65])["mask_words"].tolist() == [2]


class Args:
    """A well-formed call over host memory (never dereferenced as device memory): three robots — one without submaps —, five slots."""

    def __init__(self, lst=(0, 2, 4), n_sub=(2, 0, 3), n_frames=(65, 10, 130), words=(2, 1, 5), cap=4, d=3, thin=None, mean=True):
        self.P = frame_select_params(thin, mean)
        self.robots = session_frame_robots([6, 3, 9][:len(n_sub)], n_sub, n_frames, words)
        self.R, self.cap, self.d = len(n_sub), cap, d
        S, Nf, N = int(np.sum(n_sub)), int(np.sum(n_frames)), 18
        self.lst = None if lst is None else np.array(lst, dtype=np.int32)
        self.L = 0 if lst is None else len(lst)
        self.a = dict(count=np.zeros(max(S, 1), np.int32), src=np.zeros(max(S, 1) * cap, np.int32), seg_times=np.zeros((N, 2)), frame_times=np.zeros(max(Nf, 1)),
                      frame_pos=np.zeros((max(Nf, 1), 3)), frame_desc=np.zeros((max(Nf, 1), d)), mask=np.zeros(64, np.uint64), n_sel=np.zeros(max(S, 1), np.int32),
                      span=np.zeros((max(S, 1), 2)), mean=np.zeros((max(S, 1), d)), changed=np.zeros(max(self.L, 1), np.int32))

    def call(self, lib, host, ctx=None):
        p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
        a = self.a
        fn = lib.roman_session_frame_select_list if host else lib.roman_session_frame_select_list_dev
        return fn(ctx, None if self.P is None else C.byref(self.P), self.R, p(self.robots), self.cap, p(a["count"]), p(a["src"]), p(a["seg_times"]),
                  p(a["frame_times"]), p(a["frame_pos"]), self.d, p(a["frame_desc"]), self.L, p(self.lst), p(a["mask"]), p(a["n_sel"]), p(a["span"]),
                  p(a["mean"]), p(a["changed"]))


def check_error_codes(lib, h):
    """Every refusal of the header's list, for both entry points, on the context `h` (None: the arguments are judged first)."""
    E = _abi

    def code(edit, host, **kw):
        a = Args(**kw); edit(a)
        return a.call(lib, host, h)

    def attr(name, value):
        return lambda a: setattr(a, name, value)

    def rob(r, name, value):
        return lambda a: a.robots[name].__setitem__(r, value)

    def err():
        return lib.roman_last_error(h)
    for host in (False, True):
        # what frame_select_check refuses
        assert code(attr("P", None), host) == E.ROMAN_E_INVALID and b"fparams is NULL" in err()
        assert code(attr("d", -1), host) == E.ROMAN_E_INVALID
        assert code(attr("cap", 0), host) == E.ROMAN_E_INVALID and b"cap must be >= 1" in err()
        assert code(lambda a: a.P.reserved.__setitem__(1, 7), host) == E.ROMAN_E_INVALID and b"roman_frame_select_params_t reserved" in err()
        assert code(lambda a: None, host, thin=-1.0) == E.ROMAN_E_INVALID and b"thin_dist" in err()
        assert code(lambda a: None, host, thin=float("nan")) == E.ROMAN_E_INVALID and b"thin_dist" in err()
        assert code(attr("d", 0), host) == E.ROMAN_E_INVALID and b"want_mean" in err()
        # the robots
        assert code(attr("R", -1), host) == E.ROMAN_E_INVALID and b"R < 0" in err()
        assert code(attr("robots", None), host) == E.ROMAN_E_INVALID and b"robots is NULL" in err()
        assert code(lambda a: a.robots["reserved"].__setitem__((2, 0), 1), host) == E.ROMAN_E_INVALID and b"roman_session_frame_robot_t reserved" in err()
        for name in ("seg0", "mask_off", "n_seg", "sub0", "n_sub", "frame0", "n_frames", "mask_words"):
            assert code(rob(0, name, -1), host) == E.ROMAN_E_INVALID and b"negative" in err(), name
        assert code(rob(0, "mask_words", 1), host) == E.ROMAN_E_INVALID and b"mask_words=1" in err()                 # 65 frames need 2 words
        assert code(rob(2, "mask_words", 2), host) == E.ROMAN_E_INVALID and b"mask_words=2" in err()                 # 130 frames need 3
        for name, bad in (("seg0", 5), ("sub0", 1), ("frame0", 64), ("mask_off", 3)):
            assert code(rob(1, name, bad), host) == E.ROMAN_E_INVALID and b"not ascending and disjoint" in err(), name
        # the order: the parameter block in front of the robots, the robots in front of the list
        assert code(lambda a: (setattr(a, "cap", 0), rob(0, "mask_words", 1)(a)), host, lst=(4, 0)) == E.ROMAN_E_INVALID and b"cap must be" in err()
        assert code(rob(0, "mask_words", 1), host, lst=(4, 0)) == E.ROMAN_E_INVALID and b"mask_words=1" in err()
        # the list
        assert code(attr("L", -1), host) == E.ROMAN_E_INVALID and b"L < 0" in err()
        assert code(attr("lst", None), host) == E.ROMAN_E_INVALID and b"list is NULL" in err()
        for bad in ((0, 2, 5), (-1, 2, 4)):
            assert Args(lst=bad).call(lib, host, h) == E.ROMAN_E_INVALID and b"outside the 5 slots" in err(), bad
        for bad in ((0, 2, 2), (2, 0, 4)):
            assert Args(lst=bad).call(lib, host, h) == E.ROMAN_E_INVALID and b"not strictly ascending" in err(), bad
        assert code(rob(2, "sub0", 3), host, lst=(2,)) == E.ROMAN_E_INVALID and b"between the slots" in err()          # a gap between two robots' slots
        assert Args(lst=(0,), n_sub=(0, 0, 0)).call(lib, host, h) == E.ROMAN_E_INVALID                                # no slot at all: every entry is outside
        assert Args(lst=(0,), n_sub=(), n_frames=(), words=()).call(lib, host, h) == E.ROMAN_E_INVALID                # R == 0
        # the sizes, then the pointers
        assert code(rob(2, "n_sub", 1 << 30), host) == E.ROMAN_E_TOO_LARGE
        for name in ("count", "src", "n_sel", "span", "changed", "mask", "mean", "seg_times", "frame_times", "frame_desc"):
            assert code(lambda a: a.a.__setitem__(name, None), host) == E.ROMAN_E_INVALID and b"NULL" in err(), name
        assert code(lambda a: a.a.__setitem__("frame_pos", None), host, thin=0.5) == E.ROMAN_E_INVALID and b"frame_pos" in err()


def test_error_codes_without_a_device():
    """The arguments are judged before the context: with a NULL context a refused call answers with ITS code; a well-formed one — an
    empty list, L == 0 with a NULL list and NULL arrays, R == 0, a robot without frames — passes every check and is stopped by the
    context alone."""
    lib = _abi.load_library()
    check_error_codes(lib, None)
    bare = Args(lst=None)
    bare.a = {k: None for k in bare.a}
    for host in (False, True):
        for ok in (Args(), Args(lst=()), Args(lst=None), bare, Args(lst=(0, 1, 2, 3, 4)), Args(lst=(), n_sub=(), n_frames=(), words=()),
                   Args(n_frames=(65, 0, 130), words=(2, 0, 3)), Args(words=(4, 3, 5)), Args(thin=0.0, mean=False, d=0)):
            assert ok.call(lib, host) == _abi.ROMAN_E_INVALID
            assert b"ctx is NULL" in lib.roman_last_error(None)
