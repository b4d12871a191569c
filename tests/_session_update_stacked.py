"""A growing session with stacked frame descriptors — TEST INFRASTRUCTURE shared by the tests of
roman_session_stacked_sim_list*.

`SessionUpdateStackedListStubContext` is tests/_session_update.SessionUpdateStackedStubContext plus
roman_session_stacked_sim_list_dev: it fills the dense buffer with NaN and writes only the listed entries, each from
tests/_frame_desc_oracle.stacked_sim_oracle over that pair's two mask rows alone — an entry the gate reads without its being
listed is a NaN in similarity_mat.  `listed_oracle()` is that per-pair expectation on its own."""
import numpy as np

import _frame_desc_oracle as fo
import _session as ss
import _session_stacked as sst
import _session_update as su
from _stub_context import _view


def listed_oracle(desc, mask_words, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, pair_list, sim):
    """Writes the listed pairs' entries of the dense `sim` (pair_off[nb],) in place, one oracle call per pair."""
    blk = np.asarray(blocks).reshape(-1, 4)
    counts = np.diff(sub_off)
    for b, i, j in np.asarray(pair_list).reshape(-1, 3).tolist():
        r0, r1 = int(blk[b, 0]), int(blk[b, 1])
        side = []
        for r, k in ((r0, i), (r1, j)):
            row = sst.view_masks(mask_words, mask_off[r], int(counts[r]), frame_n[r])[k]
            side.append((np.asarray(desc)[int(frame_lo[r]):int(frame_lo[r]) + int(frame_n[r])], [fo.unpack_mask(row)]))
        sim[int(pair_off[b]) + i * int(counts[r1]) + j] = fo.stacked_sim_oracle(side[0][0], side[0][1], side[1][0], side[1][1])[0, 0]
    return sim


class SessionUpdateStackedListStubContext(su.SessionUpdateStackedStubContext):
    """Stacked frame descriptors over the pair list: roman_session_stacked_sim_list_dev in front of the list gate."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.sim_lists = []

    def session_stacked_sim_list_dev(self, d, Nf, desc_ptr, mask_ptr, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, pair_list,
                                     frame_lo_ptr, frame_n_ptr, mask_off_ptr, sub_off_ptr, blocks_ptr, pair_off_ptr, list_ptr, sim_ptr):
        self.order.append("session_stacked_sim_list")
        R, nb = len(sub_off) - 1, len(blocks)
        for host, dev_ptr, dt in ((frame_lo, frame_lo_ptr, np.int32), (frame_n, frame_n_ptr, np.int32), (mask_off, mask_off_ptr, np.int64),
                                  (sub_off, sub_off_ptr, np.int32), (blocks, blocks_ptr, np.int32), (pair_off, pair_off_ptr, np.int64)):
            host = np.asarray(host)
            assert host.dtype == dt and np.array_equal(_view(dev_ptr, host.shape, dt), host), "the device copy of a table differs from the host copy"
        assert len(frame_lo) == len(frame_n) == len(mask_off) == R and len(pair_off) == nb + 1
        counts = np.diff(sub_off)
        assert np.array_equal(pair_off, ss.tables(counts.tolist(), [tuple(b[:3]) for b in np.asarray(blocks).tolist()])[2])
        lst = np.asarray(pair_list)
        L = len(lst)
        assert lst.dtype == np.int32 and lst.shape == (L, 3) and np.array_equal(_view(list_ptr, (L, 3), np.int32), lst)
        keys = [tuple(x) for x in lst.tolist()]
        assert keys == sorted(set(keys)), "the list is not strictly ascending"
        self.sim_lists.append(lst.copy())
        words = int(max([int(mask_off[r]) + int(counts[r]) * ((int(frame_n[r]) + 63) // 64) for r in range(R)], default=0))
        desc = _view(desc_ptr, (Nf, d), np.float64) if Nf else np.zeros((0, d))
        mask = _view(mask_ptr, (words,), np.uint64) if words else np.zeros(0, np.uint64)
        sim = _view(sim_ptr, (int(pair_off[-1]),), np.float64)
        sim[:] = np.nan                                      # (the device leaves these as they are: nothing may read them)
        listed_oracle(desc, mask, frame_lo, frame_n, mask_off, sub_off, blocks, pair_off, lst, sim)
