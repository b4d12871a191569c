"""Segment tables from point clouds without a GPU: the oracle against the reference's formulas, the ABI struct
against the header, SegmentClouds and the refusals of MapTable.from_point_clouds, and every registration's column map."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import _segment_shapes_oracle as so
from conftest import ROOT
from roman_amd import _abi
from roman_amd.align import DistRegWithPruning, MinimalSegment, RansacReg, SegmentClouds, SubmapAlignParams
from roman_amd.align.segment_clouds import shape_columns
from roman_amd.align.submaps import MapTable

HEADER = os.path.join(ROOT, "include", "roman_hip.h")
METHODS = ['clipper', 'gravity', 'pcavolgrav', 'extentvolgrav', 'roman', 'sevg', 'spv', 'semanticgrav', 'clipper+prune', 'ransac']


def box_cloud(rng, n, sides, shift):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return (rng.uniform(-0.5, 0.5, (n, 3)) * sides) @ q.T + np.asarray(shift)


def test_oracle_matches_the_reference_formulas_near_the_origin():
    rng = np.random.default_rng(0)
    for n in (5, 40, 700):
        p = box_cloud(rng, n, (0.3, 1.1, 2.7), (0.4, -0.2, 0.1))
        o = so.segment(p)
        mean, cov, ratios = so.reference_formulas(p)
        assert np.allclose(o["mean"], mean, rtol=0, atol=1e-14)
        assert np.allclose(o["cov"], cov, rtol=0, atol=1e-13 * o["eig"][0])
        assert np.allclose(o["ratios"], ratios, rtol=0, atol=1e-12)
    p = box_cloud(rng, 9, (1, 1, 1), (0, 0, 0))
    bm = so.segment(p, "bottom_middle")["center"]
    assert np.array_equal(bm[:2], np.median(p[:, :2], axis=0)) and bm[2] == p[:, 2].min()
    assert np.array_equal(so.segment(p[:4])["extent"], np.zeros(3)) and so.segment(p[:4])["volume"] == 0.0


def test_far_from_the_origin_the_one_pass_form_leaves_the_device_tolerance():
    """The stated deviation, pinned: for a 0.2 m cloud at (8000, -6000, 40) m the reference's float64 one-pass
    covariance differs from the centred one by MORE than the bound the device is held to."""
    rng = np.random.default_rng(3)
    p = box_cloud(rng, 200, (0.2, 0.12, 0.05), (8000.0, -6000.0, 40.0))
    o = so.segment(p)
    _, _, ratios = so.reference_formulas(p)
    assert np.max(np.abs(ratios - o["ratios"])) > 100 * so.bounds(p, _abi.ROMAN_SEG_BLOCK_MIN)["ratio"]


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in _abi.RomanSegmentShapeParams._fields_]
    assert fields == ["center_ref", "out_stride", "col_center", "col_pca", "col_volume", "col_extent", "reserved"]
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(roman_segment_shape_params_t, {f}));' for f in fields)
    consts = "\n".join(f'printf("{k} %d\\n", {k});' for k in ("ROMAN_CENTER_MEAN", "ROMAN_CENTER_BOTTOM_MIDDLE", "ROMAN_SEG_EMPTY", "ROMAN_SEG_FEW_POINTS",
                                                                "ROMAN_SEG_DEGENERATE", "ROMAN_SEG_BLOCK_MIN"))
    prog = tmp_path / "layout.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{\n'
                    f'printf("sizeof %zu\\n", sizeof(roman_segment_shape_params_t));\n{body}\n{consts}\nreturn 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == C.sizeof(_abi.RomanSegmentShapeParams) == _abi.SEGMENT_SHAPE_PARAMS_NBYTES == 32
    for f in fields:
        assert int(out[f]) == getattr(_abi.RomanSegmentShapeParams, f).offset, f
    for k in ("ROMAN_CENTER_MEAN", "ROMAN_CENTER_BOTTOM_MIDDLE", "ROMAN_SEG_EMPTY", "ROMAN_SEG_FEW_POINTS", "ROMAN_SEG_DEGENERATE", "ROMAN_SEG_BLOCK_MIN"):
        assert int(out[k]) == getattr(_abi, k), k
    src = open(os.path.join(ROOT, "roman_amd", "csrc", "kernels.hip.h")).read()
    assert f"constexpr int SEG_BLOCK_MIN = {_abi.ROMAN_SEG_BLOCK_MIN};" in src
    hdr = open(HEADER).read()
    assert "[REF roman/map/map.py:258-262]" in hdr and "[REF roman/object/segment.py:496-508]" in hdr


def test_entry_points_exported_and_refuse_a_null_context():
    lib = _abi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.lib_path()], text=True)
    for s, nargs in {"roman_segment_shapes_dev": 8, "roman_segment_shapes": 7, "roman_ctx_set_segment_block_min": 2}.items():
        assert s in _abi.EXPORTED_SYMBOLS and len(getattr(lib, s).argtypes) == nargs and f" T {s}" in out
    P = _abi.RomanSegmentShapeParams()
    assert lib.roman_segment_shapes(None, None, None, 0, C.byref(P), None, None) == _abi.ROMAN_E_INVALID
    assert b"ctx is NULL" in lib.roman_last_error(None)
    assert lib.roman_segment_shapes_dev(None, None, None, None, 0, C.byref(P), None, None) == _abi.ROMAN_E_INVALID


def segment_stub(i, n, d=8, rng=None):
    rng = rng or np.random.default_rng(i)
    v = rng.normal(size=d)
    return SimpleNamespace(points=None if n is None else rng.normal(size=(n, 3)), id=100 + i, first_seen=float(i), last_seen=i + 2.5,
                           semantic_descriptor=v / np.linalg.norm(v))


def test_segment_clouds_from_segments():
    segs = [segment_stub(0, 5), segment_stub(1, None), segment_stub(2, 0), segment_stub(3, 12)]
    c = SegmentClouds.from_segments(segs)
    assert len(c) == 4 and c.seg_off.tolist() == [0, 5, 5, 5, 17] and c.points.shape == (17, 3) and c.points.dtype == np.float64
    assert c.ids.tolist() == [100, 101, 102, 103] and c.times.tolist() == [[0.0, 2.5], [1.0, 3.5], [2.0, 4.5], [3.0, 5.5]]
    assert c.descriptors.shape == (4, 8) and np.array_equal(c.points[5:], segs[3].points)
    segs[1].semantic_descriptor = None
    assert SegmentClouds.from_segments(segs).descriptors is None
    e = SegmentClouds.from_segments([])
    assert len(e) == 0 and e.points.shape == (0, 3) and e.seg_off.tolist() == [0]


def test_refusals_come_before_any_context(monkeypatch):
    """Every refusal is a ValueError raised while NO context exists: the stub context of tests/_stub_context.py that is handed in
    records no call and no synchronisation, and the process-wide default context — what a registration without one would make —
    must not be asked for either (it is replaced by a function that fails)."""
    import dataclasses
    import roman_amd.align.object_registration as oreg
    import roman_amd.runtime as rt
    from _stub_context import OracleContext

    def no_default_context(*a, **k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(rt, "default_context", no_default_context)
    monkeypatch.setattr(oreg, "default_context", no_default_context)
    monkeypatch.setattr(rt, "Context", no_default_context)
    good = SegmentClouds.from_segments([segment_stub(i, 6 + i) for i in range(3)])
    bad = [
        (dataclasses.replace(good, seg_off=np.array([0, 9, 6, 21])), {}),
        (dataclasses.replace(good, seg_off=np.array([0, 6, 13, 20])), {}),
        (dataclasses.replace(good, seg_off=np.array([1, 6, 13, 21])), {}),
        (dataclasses.replace(good, points=good.points[:, :2]), {}),
        (dataclasses.replace(good, points=np.array([["a", "b", "c"]] * 21, dtype=object)), {}),
        (dataclasses.replace(good, descriptors=None), {}),
        (dataclasses.replace(good, descriptors=good.descriptors[:, :5]), {}),
        (good, dict(volume=np.zeros(2))), (good, dict(extent=np.zeros((3, 2)))), (good, dict(center_ref="top")),
    ]
    regs = [SubmapAlignParams(method="roman", semantics_dim=8).get_object_registration(),
            SubmapAlignParams(method="clipper+prune").get_object_registration().on_device(8)]
    for reg in regs:
        for clouds, kw in bad:
            stub = OracleContext(n_objects=3)
            for ctx in (stub, None):                             # a context handed in, and none (the registration would make the default one)
                with pytest.raises(ValueError):
                    MapTable.from_point_clouds(reg, clouds, ctx=ctx, device="cpu", **kw)
            assert stub.calls == [] and stub.syncs == 0 and reg._ctx is None


class RecordingContext:
    """Takes the call of from_point_clouds on CPU tensors: records the block and writes sentinels where it points."""
    device = 0
    SENT = dict(center=(11.0, 12.0, 13.0), pca=(21.0, 22.0, 23.0), volume=(31.0,), extent=(41.0, 42.0, 43.0))

    def segment_shapes_dev(self, points_ptr, seg_off_ptr, seg_off, sparams, out_ptr, status_ptr):
        from _stub_context import _view
        self.params, N = sparams, len(seg_off) - 1
        out = _view(out_ptr, (N, sparams.out_stride), np.float64)
        for key, col in (("center", sparams.col_center), ("pca", sparams.col_pca), ("volume", sparams.col_volume), ("extent", sparams.col_extent)):
            if col >= 0:
                out[:, col:col + len(self.SENT[key])] = self.SENT[key]

    def sync(self):
        pass


@pytest.mark.parametrize("method", METHODS + ["clipper+prune/on_device"])
def test_column_map_is_where_pack_puts_the_attributes(method):
    d = 8
    reg = SubmapAlignParams(method=method.split("/")[0], semantics_dim=d).get_object_registration()
    if method.endswith("on_device"):
        reg = reg.on_device(d)
    clouds = SegmentClouds.from_segments([segment_stub(i, 6) for i in range(3)])
    ctx = RecordingContext()
    table = MapTable.from_point_clouds(reg, clouds, ctx=ctx, device="cpu")
    S = RecordingContext.SENT
    segs = [MinimalSegment(clouds.ids[i], S["center"], S["volume"][0], *S["pca"], S["extent"][::-1], clouds.descriptors[i], *clouds.times[i]) for i in range(3)]
    want = MapTable.from_segments(reg, segs)
    assert table.feats.tobytes() == want.feats.tobytes() and table.feats.shape == want.feats.shape
    assert table.times.tobytes() == want.times.tobytes() and table.ids.tobytes() == want.ids.tobytes()
    assert (table.point_dim, table.desc_dim, table.invariant) == (want.point_dim, want.desc_dim, want.invariant)
    cols = shape_columns(reg, d)
    assert (ctx.params.out_stride, ctx.params.col_center, ctx.params.col_pca, ctx.params.col_volume, ctx.params.col_extent) == \
        (cols.stride, 0, cols.pca, cols.volume, cols.extent) and ctx.params.center_ref == _abi.ROMAN_CENTER_MEAN
    back = clouds.minimal_segments(table)
    assert len(back) == 3 and np.array_equal(back[0].center.reshape(-1), S["center"]) and back[1].id == 101
