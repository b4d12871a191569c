"""pipeline._runs: the skipped problems of a chunked issue as runs of consecutive indices of at most `chunk` (what issue_chunked and
issue_mno_chunked issue again)."""
import numpy as np
import pytest

from roman_amd.align.pipeline import _runs


@pytest.mark.parametrize("skipped, chunk, want", [
    ([], 4, []),                                                   # nothing skipped
    ([7], 4, [(7, 8)]),                                            # one index
    ([3, 4, 5, 6, 7, 8, 9], 3, [(3, 6), (6, 9), (9, 10)]),         # a run longer than chunk: cut exactly at chunk
    ([2, 3, 4, 5], 4, [(2, 6)]),                                   # a run of exactly chunk stays whole
    ([0, 1, 3, 4], 8, [(0, 2), (3, 5)]),                           # two runs with a gap of one
    ([0, 1, 2, 5], 1, [(0, 1), (1, 2), (2, 3), (5, 6)]),           # chunk = 1
])
def test_runs(skipped, chunk, want):
    got = list(_runs(np.array(skipped, dtype=np.int64), chunk))
    assert got == want
    assert all(type(lo) is int and type(hi) is int for lo, hi in got)
    assert [b for lo, hi in got for b in range(lo, hi)] == skipped             # every skipped problem once, in order, nothing else
