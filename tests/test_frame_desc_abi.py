"""The C-ABI boundary of the frame-descriptor entry points (include/roman_hip.h) without a GPU: exported and
declared symbols, struct layout against the header, and every argument check that runs before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from roman_amd import _abi
from roman_amd.runtime import frame_select_params, grid_gate_params

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
ENTRY_POINTS = {"roman_frame_select_dev": 17, "roman_frame_select": 17, "roman_stacked_sim_dev": 11, "roman_stacked_sim": 11,
                "roman_grid_gate_sim_dev": 21, "roman_grid_gate_sim": 21, "roman_ctx_set_stacked_band": 2}


def test_entry_points_exported_and_declared():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    src = open(HEADER).read()
    for s, nargs in ENTRY_POINTS.items():
        assert s in _abi.EXPORTED_SYMBOLS and s in lib._roman_symbols
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, s
        assert f" T {s}" in out, f"{s} is not an exported text symbol of the built library"
        proto = src[src.index(f"ROMAN_API int {s}("):]
        assert proto[:proto.index(");")].count(",") + 1 == nargs, s
    assert "[REF roman/map/map.py:210-242]" in src and "[REF roman/map/map.py:155-162]" in src
    # the scope comments no longer leave these modes with the caller
    assert "stacked frame descriptors and the" not in src and "roman_stacked_sim_dev and roman_grid_gate_sim_dev below" in src


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.RomanFrameSelectParams._fields_]
    assert fields == ["thin", "want_mean", "thin_dist", "reserved"]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(roman_frame_select_params_t, {f}));' for f in fields)
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof %zu\\n", sizeof(roman_frame_select_params_t));\n{body}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == C.sizeof(_abi.RomanFrameSelectParams) == _abi.FRAME_SELECT_PARAMS_NBYTES == 24
    for f in fields:
        assert int(out[f]) == getattr(_abi.RomanFrameSelectParams, f).offset, f
    assert C.sizeof(_abi.RomanGridGateParams) == 56                      # the gate's block is the one roman_grid_gate_dev takes


def test_bad_arguments_are_refused_without_a_device():
    """NULL context: an error code, not a crash (the checks run before anything touches the GPU)."""
    lib = _abi.load_library()
    v = C.c_void_p(np.zeros(8, np.int64).ctypes.data)
    fp, gp = frame_select_params(), grid_gate_params(5.0)
    for fn in (lib.roman_frame_select_dev, lib.roman_frame_select):
        assert fn(None, C.byref(fp), 0, 1, None, None, 0, None, 0, None, None, 0, None, None, None, None, None) == _abi.ROMAN_E_INVALID
        assert b"ctx is NULL" in lib.roman_last_error(None)
    for fn in (lib.roman_stacked_sim_dev, lib.roman_stacked_sim):
        assert fn(None, 4, 0, None, 0, None, 0, None, 0, None, None) == _abi.ROMAN_E_INVALID
    for fn in (lib.roman_grid_gate_sim_dev, lib.roman_grid_gate_sim):
        assert fn(None, C.byref(gp), 0, 0, *([None] * 8), *([v] * 9)) == _abi.ROMAN_E_INVALID
    assert lib.roman_ctx_set_stacked_band(None, 32) == _abi.ROMAN_E_INVALID
    assert _abi.ROMAN_E_NOMEM == -4 and "#define ROMAN_E_NOMEM          -4" in open(HEADER).read()


def test_the_python_layer_builds_the_blocks_the_header_describes():
    fp = frame_select_params(10.0, True)
    assert (fp.thin, fp.want_mean, fp.thin_dist, fp.reserved[0], fp.reserved[1]) == (1, 1, 10.0, 0, 0)
    fp = frame_select_params(None, False)
    assert (fp.thin, fp.want_mean, fp.thin_dist) == (0, 0, 0.0)
    assert _abi.STACKED_BAND_MIN == 32
    src = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert "constexpr int STACK_TILE = 32;" in src
