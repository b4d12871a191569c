"""ObjectRegistration.mno_clipper_batch without a GPU: a CPU double with runtime.Context.mno_batch's signature computes every
problem of the packed batch with the oracle's loop, and the Python layer — packing into one feature pool, explicit association
lists, result shaping, empty maps — is checked against the per-pair definition composed from the object maps."""
import numpy as np
import pytest

from _mno_oracle import mno_from_dense, oracle_mno, plain_params, pose_of
from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.runtime import MnoResult, stats_dtype


class OracleMnoContext:
    """mno_batch() on the CPU oracle, from the arrays the C ABI would receive."""

    def __init__(self, orc):
        self.orc, self.calls = orc, []

    def mno_batch(self, params, feats, off1, n1, off2, n2, num_solutions=2, assoc=None, assoc_off=None, kmax=None):
        B, K, dim = len(n1), int(num_solutions), params.point_dim
        self.calls.append((B, K, kmax, assoc is not None))
        P = _abi.RomanParams.from_buffer_copy(params); P.invariant = _abi.ROMAN_INV_EUCLIDEAN
        out, score = [], np.zeros((B, K)); T = np.full((B, K, dim + 1, dim + 1), np.nan)
        status = np.zeros((B, K), np.int32); stats = np.zeros((B, K), stats_dtype())
        for b in range(B):
            D1 = feats[off1[b]:off1[b] + n1[b]]; D2 = feats[off2[b]:off2[b] + n2[b]]
            if n1[b] == 0 or n2[b] == 0:
                out.append([np.zeros((0, 2), np.int32) for _ in range(K)])
                status[b] = _abi.ROMAN_ST_EMPTY_MAP | _abi.ROMAN_ST_INSUFFICIENT
                continue
            A = None
            if assoc is not None and assoc_off[b + 1] > assoc_off[b]:
                A = assoc[assoc_off[b]:assoc_off[b + 1]]
            mat, Aall = self.orc.build_matrix(params, D1, D2, A)
            Mo, Co = mat.dense()
            sols = mno_from_dense(self.orc, P, Mo, Co, Aall, K)
            row = []
            for k, s in enumerate(sols):
                a = s["assoc"].astype(np.int32)
                score[b, k] = s["score"]
                if len(a) > kmax:
                    status[b, k] |= _abi.ROMAN_ST_ASSOC_TRUNCATED
                if len(a) >= dim:
                    T[b, k] = self.orc.t_align(D1[a[:, 0], :dim], D2[a[:, 1], :dim], dim)
                else:
                    status[b, k] |= _abi.ROMAN_ST_INSUFFICIENT
                row.append(a[:kmax])
            out.append(row)
        return MnoResult(out, score, T, status, stats)


@pytest.mark.parametrize("method,d", [("clipper", 0), ("roman", 16), ("clipper+prune", 16)])
def test_mno_clipper_batch_equals_the_per_pair_definition(orc, method, d):
    kw = dict(cosine_min=0.5) if method == "clipper+prune" else (dict(semantics_dim=d) if method == "roman" else {})
    reg = registration_for(method, **kw)
    pairs = []
    for k, (n, m) in enumerate([(12, 14), (9, 8), (0, 7), (15, 11)]):
        pr = synth.make_pair(max(n, 1), max(m, 1), d, 700 + k)
        pairs.append((pr.map1[:n], pr.map2[:m]))
    stub = OracleMnoContext(orc)
    sols, poses, res = reg.mno_clipper_batch(pairs, num_solutions=3, return_result=True, ctx=stub)
    assert stub.calls == [(4, 3, 12, method == "clipper+prune")]
    assert len(sols) == len(poses) == 4 and res.status.shape == (4, 3)
    for b, (m1, m2) in enumerate(pairs):
        assert len(sols[b]) == 3 and len(poses[b]) == 3
        if len(m1) == 0 or len(m2) == 0:
            for k in range(3):
                Ain, score = sols[b][k]
                assert Ain.shape == (0, 2) and Ain.dtype == np.int64 and score == 0 and np.all(np.isnan(poses[b][k]))
                assert res.status[b, k] & _abi.ROMAN_ST_EMPTY_MAP
            continue
        ref = oracle_mno(orc, reg, m1, m2, 3)
        for k in range(3):
            Ain, score = sols[b][k]
            assert Ain.dtype == np.int64 and Ain.ndim == 2 and Ain.shape[1] == 2
            assert np.array_equal(Ain, ref[k]["assoc"]) and abs(score - ref[k]["score"]) < 1e-9
            if len(Ain) >= 3:
                assert np.linalg.norm(poses[b][k] - pose_of(orc, m1, m2, Ain)) < 1e-9
            else:
                assert np.all(np.isnan(poses[b][k])) and res.status[b, k] & _abi.ROMAN_ST_INSUFFICIENT


def test_explicit_lists_reach_the_call_as_one_ragged_array(orc):
    reg = registration_for("clipper+prune", cosine_min=0.5)
    from roman_amd.align import batch as rb
    pairs = [(synth.make_pair(10, 9, 16, 800 + k).map1, synth.make_pair(10, 9, 16, 800 + k).map2) for k in range(3)]
    batch = rb.batch_from_pairs(reg, pairs)
    assert batch.assoc is not None and batch.assoc_off[-1] == len(batch.assoc)
    seen = {}

    class Spy(OracleMnoContext):
        def mno_batch(self, params, feats, off1, n1, off2, n2, num_solutions=2, assoc=None, assoc_off=None, kmax=None):
            seen.update(assoc=assoc, assoc_off=assoc_off, kmax=kmax, K=num_solutions)
            return super().mno_batch(params, feats, off1, n1, off2, n2, num_solutions, assoc, assoc_off, kmax)

    res = rb.run_mno_batch(reg, batch, num_solutions=2, ctx=Spy(orc))
    assert np.array_equal(seen["assoc"], batch.assoc) and np.array_equal(seen["assoc_off"], batch.assoc_off) and seen["kmax"] == 9 and seen["K"] == 2
    assert len(res.assoc) == 3 and all(len(r) == 2 for r in res.assoc)
