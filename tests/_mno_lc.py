"""The hypothesis tail (roman_mno_lc_tail_dev) stated on the host: tests/_lc_tail.lc_tail over the flattened B*K poses with the
per-problem inputs repeated K times, then the best rule and both accepted lists in NumPy."""
import dataclasses

import numpy as np

from roman_amd import _abi
from roman_amd.runtime import LcInputs

import _lc_tail as lt

NOT_A_CANDIDATE = _abi.ROMAN_LC_FAILED | _abi.ROMAN_LC_SKIPPED | _abi.ROMAN_LC_INTERNAL


def repeated(lc: LcInputs, K):
    """The LcInputs of the flattened call: every per-problem array repeated K times (the frame pools stay)."""
    rep = lambda a: None if a is None else np.repeat(np.asarray(a), K, axis=0)
    return dataclasses.replace(lc, T_ref=rep(lc.T_ref), enable=rep(lc.enable), iL=rep(lc.iL), iR=rep(lc.iR))


def best_rule(records, B, K):
    """-> (B,) int32: among a problem's records without FAILED_* / SKIPPED / INTERNAL the largest n_assoc, the lower k among
    equals; -1 when there is none."""
    flags = records["flags"].reshape(B, K); n = records["n_assoc"].reshape(B, K).astype(np.int64)
    key = np.where((flags & NOT_A_CANDIDATE) == 0, n, -1)
    best = np.argmax(key, axis=1).astype(np.int32) if B else np.zeros(0, np.int32)       # argmax: the FIRST maximum
    best[key.max(axis=1, initial=-1) < 0] = -1
    return best


def lists(records, best, B, K):
    flags = records["flags"].reshape(B, K)
    acc = np.nonzero(flags.reshape(-1) & _abi.ROMAN_LC_ACCEPTED)[0].astype(np.int32)
    has = best >= 0
    pick = flags[np.arange(B), np.maximum(best, 0)]
    acc_best = np.nonzero(has & ((pick & _abi.ROMAN_LC_ACCEPTED) != 0))[0].astype(np.int32)
    return acc, acc_best


def mno_lc_tail(lc: LcInputs, K, T, n_assoc, status):
    """T: (B, K, dim+1, dim+1); n_assoc, status: (B, K).  -> (records (B*K,), best (B,), accepted, accepted_best)."""
    status = np.asarray(status, dtype=np.int32); B = status.shape[0]
    s = lc.dim + 1
    rec, _ = lt.lc_tail(repeated(lc, K), np.asarray(T, dtype=np.float64).reshape(B * K, s, s), np.asarray(n_assoc).reshape(B * K), status.reshape(B * K))
    best = best_rule(rec, B, K)
    acc, acc_best = lists(rec, best, B, K)
    return rec, best, acc, acc_best


# ---------------------------------------------------------------------------------------------
# the three calls on a stand-in context (tests/_stub_context.OracleContext's idiom: raw addresses in, results through them)
# ---------------------------------------------------------------------------------------------
class MnoLcCalls:
    """mno_batch_dev through the oracle's mno loop (tests/_mno_oracle.py), mno_lc_tail_dev through mno_lc_tail() above,
    mno_lc_batch_dev as the two in a row.  Mixed into an OracleContext (self.orc, self.n_objects, self.dim).  `mno_skip_once`:
    problems (by (off1, off2)) reported ROMAN_ST_WORKSPACE on their first appearance; `mno_tail_inputs`: what every tail call read."""

    def mno_batch_dev(self, P, feats_ptr, F, off1, n1, off2, n2, K, kmax, a_ptr, sol_ptr, stats_ptr=None, assoc_ptr=None, assoc_off=None):
        from _mno_oracle import mno_from_dense
        from _stub_context import _view
        from roman_amd.runtime import mno_solution_dtype
        B, d = len(n1), self.dim
        self.__dict__.setdefault("mno_calls", []).append(B)
        if hasattr(self, "order"):
            self.order.append("mno")
        skip = self.__dict__.setdefault("mno_skip_once", set())
        rows = max(int(np.max(np.asarray(off1) + np.asarray(n1))), int(np.max(np.asarray(off2) + np.asarray(n2))), self.n_objects) if B else 0
        feats = _view(feats_ptr, (rows, F), np.float64)
        a_out = _view(a_ptr, (B, K, kmax, 2), np.int32); sol = _view(sol_ptr, (B, K), mno_solution_dtype())
        Pp = _abi.RomanParams.from_buffer_copy(P); Pp.invariant = _abi.ROMAN_INV_EUCLIDEAN
        for b in range(B):
            key = (int(off1[b]), int(off2[b]))
            sol[b]["n_assoc"] = 0; sol[b]["score"] = 0.0; sol[b]["T"] = np.nan; a_out[b] = -1
            if key in skip:
                skip.discard(key); sol[b]["status"] = _abi.ROMAN_ST_WORKSPACE
                continue
            D1 = feats[off1[b]:off1[b] + n1[b]]; D2 = feats[off2[b]:off2[b] + n2[b]]
            if len(D1) == 0 or len(D2) == 0:
                sol[b]["status"] = _abi.ROMAN_ST_EMPTY_MAP | _abi.ROMAN_ST_INSUFFICIENT
                continue
            mat, A = self.orc.build_matrix(P, D1, D2, None)
            Mo, Co = mat.dense()
            for k, s in enumerate(mno_from_dense(self.orc, Pp, Mo, Co, A, K)):
                a = s["assoc"].astype(np.int32)
                sol[b, k]["n_assoc"] = min(len(a), kmax); a_out[b, k, :min(len(a), kmax)] = a[:kmax]; sol[b, k]["score"] = s["score"]
                if len(a) >= d:
                    sol[b, k]["T"][:(d + 1) ** 2] = self.orc.t_align(D1[a[:, 0], :d], D2[a[:, 1], :d], d).ravel(); sol[b, k]["status"] = 0
                else:
                    sol[b, k]["status"] = _abi.ROMAN_ST_INSUFFICIENT

    def mno_lc_tail_dev(self, lp, B, K, sol_ptr, rec_ptr, best_ptr, idx_ptr, cnt_ptr, bidx_ptr, bcnt_ptr, T_ref_ptr=None, enable_ptr=None,
                        FL_ptr=None, iL_ptr=None, FR_ptr=None, iR_ptr=None):
        from _stub_context import _view
        from roman_amd.runtime import lc_record_dtype, mno_solution_dtype
        if hasattr(self, "order"):
            self.order.append("mno_tail")
        s = int(lp.dim) + 1
        sol = _view(sol_ptr, (B, K), mno_solution_dtype())
        assert not np.any(sol["status"] & _abi.ROMAN_ST_WORKSPACE), "the tail saw a skipped attempt"
        iL, iR = _view(iL_ptr, (B,), np.int32), _view(iR_ptr, (B,), np.int32)
        lc = LcInputs(dim=int(lp.dim), force_rm_upside_down=bool(lp.force_rm_upside_down), force_rm_lc_roll_pitch=bool(lp.force_rm_lc_roll_pitch),
                      tilt_thresh=None if lp.tilt_thresh < 0 else float(lp.tilt_thresh), lc_association_thresh=int(lp.lc_association_thresh),
                      T_ref=_view(T_ref_ptr, (B, 4, 4), np.float64).copy(), enable=_view(enable_ptr, (B,), np.int32).copy(),
                      FL=_view(FL_ptr, (int(iL.max()) + 1, 4, 4), np.float64).copy(), iL=iL.copy(),
                      FR=_view(FR_ptr, (int(iR.max()) + 1, 4, 4), np.float64).copy(), iR=iR.copy())
        self.__dict__.setdefault("mno_tail_inputs", []).append(lc)
        rec, best, acc, acc_best = mno_lc_tail(lc, K, sol["T"][:, :, :s * s].reshape(B, K, s, s), sol["n_assoc"], sol["status"])
        _view(rec_ptr, (B * K,), lc_record_dtype())[:] = rec; _view(best_ptr, (B,), np.int32)[:] = best
        _view(idx_ptr, (B * K,), np.int32)[:len(acc)] = acc; _view(cnt_ptr, (1,), np.int32)[0] = len(acc)
        _view(bidx_ptr, (B,), np.int32)[:len(acc_best)] = acc_best; _view(bcnt_ptr, (1,), np.int32)[0] = len(acc_best)

    def mno_lc_batch_dev(self, P, feats_ptr, F, off1, n1, off2, n2, K, kmax, a_ptr, sol_ptr, lp, rec_ptr, best_ptr, idx_ptr, cnt_ptr, bidx_ptr,
                         bcnt_ptr, stats_out_ptr=None, assoc_ptr=None, assoc_off=None, **tail):
        self.mno_batch_dev(P, feats_ptr, F, off1, n1, off2, n2, K, kmax, a_ptr, sol_ptr, stats_out_ptr, assoc_ptr, assoc_off)
        self.mno_lc_tail_dev(lp, len(n1), K, sol_ptr, rec_ptr, best_ptr, idx_ptr, cnt_ptr, bidx_ptr, bcnt_ptr, **tail)


def stub_context():
    """The stand-in with every call of the pools and session paths (tests/_session_aabb.py) plus the three above."""
    import _session_aabb as sab

    class MnoLcStubContext(MnoLcCalls, sab.SessionAabbStubContext):
        pass
    return MnoLcStubContext()
