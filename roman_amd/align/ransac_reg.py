"""RansacReg — the RANSAC baseline of the ROMAN paper on the HIP library.

Mirrors the plugin surface of [REF roman/align/ransac_reg.py:9-53]: one point per object (`seg.center`, 3-D only), all
len(map1) x len(map2) correspondences, three-point hypotheses with an edge-length check, inliers within 0.5 m.  The reference
delegates the search to open3d, whose sampling and early stop are reproducible neither across runs nor across machines; here
the search is the deterministic procedure of DESIGN.md §4.7 (roman_ransac_batch in include/roman_hip.h), one device call for
any number of pairs.  `T_align()` is inherited: Arun's fit on the returned correspondences.
"""
from typing import List

import numpy as np

from .. import _abi
from .object_registration import ObjectRegistration


class RansacReg(ObjectRegistration):
    """Constructor signature of [REF roman/align/ransac_reg.py:10] plus keyword-only extras: `round` (hypotheses between two
    evaluations of the stop rule), `max_dist` (the inlier distance the reference hard-codes), `confidence` (open3d's default)
    and `seed`."""

    def __init__(self, edge_len=0.95, dim=3, max_iteration=int(1e6), *, round=4096, max_dist=0.5, confidence=0.999, seed=0):
        assert dim == 3, "Only 3D points supported for RANSAC registration."
        super().__init__(dim)
        self.edge_len = edge_len
        self.max_iteration = max_iteration
        self.round = round
        self.max_dist = max_dist
        self.confidence = confidence
        self.seed = seed

    # ------------------------------------------------------------------ plumbing
    def _ransac_params(self) -> _abi.RomanRansacParams:
        p = _abi.RomanRansacParams()
        p.max_iteration = int(self.max_iteration)
        p.round = int(self.round)
        p.edge_len = float(self.edge_len)
        p.max_dist = float(self.max_dist)
        p.confidence = float(self.confidence)
        p.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return p

    def pack(self, object_map) -> np.ndarray:
        """(n, 3) float64: the centre of every object ([REF roman/align/ransac_reg.py:18-19])."""
        if len(object_map) == 0:
            return np.zeros((0, 3), dtype=np.float64)
        return np.array([np.asarray(seg.center, dtype=np.float64).reshape(-1)[:3] for seg in object_map], dtype=np.float64)

    def _association_list(self, map1, map2):
        return None                                              # always all-to-all ([REF roman/align/ransac_reg.py:27-30])

    # ------------------------------------------------------------------ reference API
    def register(self, map1: List, map2: List):
        """[REF roman/align/ransac_reg.py:16-53]: the (k, 2) inlier correspondences of the best hypothesis, (0, 2) when no
        hypothesis survived the prune."""
        if len(map1) == 0 or len(map2) == 0:
            return np.array([[]])                                # (1,0) float64, as the base class
        res = self.register_and_align_batch([(map1, map2)])
        return np.asarray(res.assoc[0], dtype=np.int32).reshape(-1, 2)

    def register_and_align_batch(self, pairs, u0=None):
        """register() + T_align() for many (map1, map2) pairs in one device call -> runtime.RansacResult."""
        if u0 is not None:
            raise ValueError("RANSAC registration has no initial vector")
        from .batch import batch_from_pairs, run_batch
        return run_batch(self, batch_from_pairs(self, pairs))

    def get_MCA(self, map1: List, map2: List):
        raise NotImplementedError("RANSAC registration builds no affinity matrix")

    def mno_clipper(self, map1: List, map2: List, num_solutions=2):
        raise NotImplementedError("RANSAC registration builds no affinity matrix")

    def mno_clipper_batch(self, pairs, num_solutions=2, return_result=False, ctx=None):
        raise NotImplementedError("RANSAC registration builds no affinity matrix")
