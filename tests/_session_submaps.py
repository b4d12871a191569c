"""The submaps of every map of a session in one call — TEST INFRASTRUCTURE shared by tests/test_session_submaps_cpu.py
and tests/test_gpu_session_submaps.py.

The expectation for roman_session_submaps* is tests/_submaps_oracle.py per map (the CPU tests) or roman_submaps_dev per map on the
same device (the GPU tests), concatenated: `OracleSessionSubmapContext` is the stand-in whose session_submaps_dev is built on that
oracle, `session_of()` concatenates R maps into the call's tables, and `RecordingSessionContext` is tests/_session.py's stand-in
for submap_align_session that also records which pool and ids addresses reach the batch and the shared-segment removal."""
import numpy as np

import _session as ss
import _submaps_oracle as so
from _stub_context import _view


def session_of(maps):
    """maps: list of (feats (N_r, F), times (N_r, 2), ids (N_r,) or None, descs (S_r,)) -> dict(seg_off, sub_off, feats, times, ids,
    descs): the R tables concatenated in map order, as the C ABI takes them."""
    from roman_amd.runtime import submap_desc_dtype
    F = maps[0][0].shape[1] if maps else 3
    seg_off = np.concatenate([[0], np.cumsum([len(m[0]) for m in maps])]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum([len(m[3]) for m in maps])]).astype(np.int32)
    cat = lambda k, tail, dt: np.ascontiguousarray(np.concatenate([np.asarray(m[k], dtype=dt).reshape((-1,) + tail) for m in maps])) if maps else np.zeros((0,) + tail, dt)
    ids = None if (not maps or maps[0][2] is None) else cat(2, (), np.int64)
    descs = np.concatenate([np.asarray(m[3], dtype=submap_desc_dtype()).reshape(-1) for m in maps]) if maps else np.zeros(0, dtype=submap_desc_dtype())
    return dict(seg_off=seg_off, sub_off=sub_off, feats=cat(0, (F,), np.float64), times=cat(1, (2,), np.float64), ids=ids, descs=descs)


class OracleSessionSubmapContext(so.OracleSubmapContext):
    """OracleSubmapContext plus session_submaps_dev: submaps_dev — submaps_oracle — per map, each over its own slices of the raw
    addresses the real entry takes, which is the call's contract restated."""

    def __init__(self):
        super().__init__()
        self.session_calls = 0

    def session_submaps_dev(self, P, F, seg_off, feats_ptr, times_ptr, sub_off, descs, pool_ptr, count_ptr, src_ptr, status_ptr, seg_ids_ptr=None,
                            ids_out_ptr=None, desc_dim=0, desc_out_ptr=None):
        self.session_calls += 1
        cap, Fo = int(P.cap), int(P.point_dim) + F - 3
        assert seg_off.dtype == np.int64 and sub_off.dtype == np.int32 and seg_off[0] == 0 and sub_off[0] == 0 and len(descs) == sub_off[-1]
        at = lambda ptr, n: (ptr + n) if ptr else None
        calls = self.calls
        for r in range(len(seg_off) - 1):
            n0, s0 = int(seg_off[r]), int(sub_off[r])
            if sub_off[r + 1] == s0:
                continue
            self.submaps_dev(P, int(seg_off[r + 1]) - n0, F, feats_ptr + 8 * F * n0, times_ptr + 16 * n0, descs[s0:int(sub_off[r + 1])],
                             pool_ptr + 8 * Fo * cap * s0, count_ptr + 4 * s0, src_ptr + 4 * cap * s0, status_ptr + 4 * s0,
                             seg_ids_ptr=at(seg_ids_ptr, 8 * n0), ids_out_ptr=at(ids_out_ptr, 8 * cap * s0), desc_dim=desc_dim,
                             desc_out_ptr=at(desc_out_ptr, 8 * desc_dim * s0))
        self.calls = calls                                   # (per-map calls of the real thing are what a test counts there)


class RecordingSessionContext(ss.SessionStubContext):
    """SessionStubContext that keeps the addresses of the pool the batch reads and of the ids the shared-segment removal reads."""

    def __init__(self, dim=3):
        super().__init__(dim)
        self.batch_pools, self.reduce_ids, self.reduce_rows = [], [], []

    def align_batch_dev(self, P, feats_ptr, *a, **kw):
        self.batch_pools.append(int(feats_ptr))
        return super().align_batch_dev(P, feats_ptr, *a, **kw)

    def shared_reduce_dev(self, B, F, feats_ptr, region_row0, ids_ptr, *a, **kw):
        self.reduce_ids.append(int(ids_ptr)); self.reduce_rows.append(int(region_row0))
        return super().shared_reduce_dev(B, F, feats_ptr, region_row0, ids_ptr, *a, **kw)


def same_pool(got, want):
    """Two SubmapPools field by field: what build_session_pools leaves for a robot against build_submap_pool for it."""
    assert got.cap == want.cap and got.descriptor_mode == want.descriptor_mode
    assert got.centers is want.centers and got.table is want.table
    for name in ("count", "src", "ids", "status"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
    assert (got.desc is None) == (want.desc is None)
    if want.desc is not None:
        assert got.desc.shape == want.desc.shape and np.array_equal(got.desc, want.desc, equal_nan=True)
    for name in ("pool", "ids_dev", "desc_dev"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), name
        if b is not None:
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.is_contiguous(), name
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name           # raw bytes: NaN rows of empty submaps included
    assert got.frames is want.frames and (got.frame_mask is None) == (want.frame_mask is None)


def one_storage(pools, field="pool"):
    """The tensors `field` of the pools lie in ONE storage, each where the one in front of it ends -> the storage's first address."""
    t = [x for x in (getattr(q, field) for q in pools) if x.numel()]          # (a robot without submaps owns no rows: nothing to place)
    base = t[0].untyped_storage().data_ptr()
    at = t[0].data_ptr()
    for x in t:
        assert x.untyped_storage().data_ptr() == base and x.data_ptr() == at, field
        at += x.numel() * x.element_size()
    return t[0].data_ptr()
