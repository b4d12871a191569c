"""The refusals of roman_shared_reduce_dev (include/roman_hip.h): each returns ROMAN_E_INVALID with a text in roman_last_error
and enqueues nothing — after ctx.sync() keep, kept and the gather region still hold their fill."""
import ctypes as C

import numpy as np
import pytest

from _hipmem import Hip
from roman_amd import _abi

pytestmark = pytest.mark.gpu

F, ROWS = 6, 20


def test_every_refusal_leaves_the_outputs_alone(ctx):
    hip = Hip()
    try:
        off1 = np.array([0, 10], dtype=np.int64); n1 = np.array([5, 4], dtype=np.int32)
        off2 = np.array([5, 14], dtype=np.int64); n2 = np.array([5, 6], dtype=np.int32)
        total = int(n1.sum() + n2.sum())
        ids = np.arange(ROWS, dtype=np.int64) % 7                                # shared ids: a call that went through would write
        feats = np.concatenate([np.arange(ROWS * F, dtype=np.float64).reshape(ROWS, F), np.full((total, F), -5.0)])
        d_feats, d_ids = hip.upload(feats), hip.upload(ids)
        d_keep, d_kept = hip.upload(np.full(total, -1, np.int32)), hip.upload(np.full((2, 2), -7, np.int32))
        lib = ctx._lib
        vp = lambda x: None if x is None else C.c_void_p(int(x))
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

        def call(h=ctx._h, B=2, F_=F, feats=d_feats, row0=ROWS, ids=d_ids, o1=off1, m1=n1, o2=off2, m2=n2, keep=d_keep, kept=d_kept):
            return lib.roman_shared_reduce_dev(h, B, F_, vp(feats), row0, vp(ids), ptr(o1), ptr(m1), ptr(o2), ptr(m2), vp(keep), vp(kept))

        neg = lambda a, v: np.array([a[0], v], dtype=a.dtype)
        cases = {
            "NULL context": dict(h=None),
            "B < 0": dict(B=-1),
            "F < 1": dict(F_=0),
            "F negative": dict(F_=-3),
            "region_row0 < 0": dict(row0=-1),
            "NULL off1": dict(o1=None), "NULL n1": dict(m1=None), "NULL off2": dict(o2=None), "NULL n2": dict(m2=None),
            "negative n1": dict(m1=neg(n1, -1)), "negative n2": dict(m2=neg(n2, -2)),
            "negative off1": dict(o1=neg(off1, -1)), "negative off2": dict(o2=neg(off2, -4)),
            "NULL feats": dict(feats=None), "NULL ids": dict(ids=None), "NULL keep": dict(keep=None), "NULL kept": dict(kept=None),
            "side 1 reaches into the region": dict(o1=neg(off1, ROWS - 3)),
            "side 2 reaches into the region": dict(o2=neg(off2, ROWS - 5)),
            "region in front of the slices": dict(row0=ROWS - 1),
        }
        for name, kw in cases.items():
            rc = call(**kw)
            assert rc == _abi.ROMAN_E_INVALID, (name, rc)
            msg = lib.roman_last_error(None if name == "NULL context" else ctx._h)
            assert msg and len(msg.strip()) > 0, name
        ctx.sync()
        assert np.all(hip.download(d_keep, (total,), np.int32) == -1) and np.all(hip.download(d_kept, (2, 2), np.int32) == -7)
        assert np.array_equal(hip.download(d_feats, feats.shape, np.float64), feats)
        # ... and the context goes on working: the same call with nothing wrong
        assert call() == 0
        ctx.sync()
        kept = hip.download(d_kept, (2, 2), np.int32)
        assert np.all(kept >= 0) and (kept[0, 0] < 5 or kept[0, 1] < 5)
        assert not np.array_equal(hip.download(d_feats, feats.shape, np.float64)[ROWS:], feats[ROWS:])
    finally:
        hip.free_all()
