"""What reaches the C ABI from the batch wrappers of roman_amd.runtime.Context, and what they make of what comes back — without
a GPU.  `CallRecorder` (a tests/_recording_lib.RecordingLib) stands behind roman_amd._abi for the 18 batch entry points: it decodes
every argument into plain data while the call is live (ENTRIES: the argument lists of include/roman_hip.h with the element
count of every host array), writes a fixed pattern through every host output pointer and returns the code the case chose.
`run_all()` drives the cases of CASES and returns one JSON-able transcript; tests/golden/make_runtime_calls_golden.py stores it,
tests/test_runtime_marshalling.py compares the tree with the stored one."""
import dataclasses
import inspect

import numpy as np

from _recording_lib import RecordingLib, _arr, _put
from roman_amd import _abi
from roman_amd import runtime as rt

METHODS = ["align_batch", "align_batch_resident", "align_batch_dev",
           "align_lc_batch", "align_lc_batch_ids", "align_lc_batch_dev", "lc_tail_dev",
           "mno_batch", "mno_batch_dev", "mno_lc_batch", "mno_lc_batch_dev", "mno_lc_tail_dev",
           "ransac_batch", "ransac_batch_dev", "ransac_lc_batch", "ransac_lc_batch_dev",
           "shared_ids_dev", "shared_reduce_dev"]
CARRIES_RESULT = ["align_batch", "align_batch_resident", "align_lc_batch", "align_lc_batch_ids"]      # .result on ROMAN_E_INTERNAL
LAST_ERROR = b"recorded failure"

# ---------------------------------------------------------------------------------------------------------------------------
# the argument lists: (name, kind) in the header's order.  Kinds: H the context, I an integer, REF a byref structure (or NULL),
# DEV a device address, ("in", dtype, count) a host input and ("out", dtype, count, fill) a host output, count / fill functions
# of the call's environment `e` (its integers by name, its host arrays through e.arr(name)).
# ---------------------------------------------------------------------------------------------------------------------------
H, I, REF, DEV = "h", "i", "ref", "dev"
i32, i64, f64 = np.int32, np.int64, np.float64


def IN(dtype, count):
    return ("in", dtype, count)


def OUT(dtype, count, fill):
    return ("out", dtype, count, fill)


def _n_assoc(e):                                                   # entries of the explicit lists / of u0
    if e.given("assoc"):
        return int(e.arr("assoc_off")[-1])
    return int((e.arr("n1").astype(np.int64) * e.arr("n2")).sum())


def _counts(n, kmax):                                              # per-problem counts that differ: 0, above kmax, inside
    return np.array([[0, kmax + 2, 1, 2][k % 4] for k in range(n)], dtype=np.int32)


def _fill_stats(e, n):
    a = np.zeros(n, dtype=rt.stats_dtype())
    a["n_assoc_in"] = 10 + np.arange(n); a["n_live"] = 20 + np.arange(n); a["nnz_upper"] = 3000000000 + np.arange(n)
    a["n_pass"] = 5; a["outer_iters"] = 6; a["inner_iters"] = 7; a["ls_trials"] = 8
    a["score"] = 0.25 + np.arange(n); a["d_final"] = 1.5 * (1 + np.arange(n))
    return a


def _fill_lc_records(e, n):
    a = np.zeros(n, dtype=rt.lc_record_dtype())
    a["problem"] = np.arange(n); a["n_assoc"] = 4 + np.arange(n); a["flags"] = 1 << (np.arange(n) % 5)
    a["T_hat"] = (0.125 * np.arange(n * 16)).reshape(n, 4, 4); a["theta"] = 0.5 + np.arange(n); a["dist"] = 2.5 * np.arange(n)
    a["edge_t"] = (1.0 + np.arange(n * 3)).reshape(n, 3); a["edge_q"] = (0.1 * (1 + np.arange(n * 4))).reshape(n, 4)
    return a


def _fill_sol(e):
    n = e.B * e.Kc
    a = np.zeros(n, dtype=rt.mno_solution_dtype())
    a["n_assoc"] = _counts(n, e.kmax); a["status"] = 3 + np.arange(n); a["score"] = 0.75 + np.arange(n)
    a["T"] = (1.0 + 0.5 * np.arange(n * 16)).reshape(n, 16)
    return a


def _fill_ransac(e):
    a = np.zeros(e.B, dtype=rt.ransac_record_dtype())
    a["n_assoc"] = _counts(e.B, e.kmax); a["status"] = 3 + np.arange(e.B); a["n_hyp"] = 40 + np.arange(e.B); a["n_scored"] = 30 + np.arange(e.B)
    a["best_hyp"] = 7 + np.arange(e.B); a["best_count"] = 5 + np.arange(e.B); a["best_sse"] = 0.5 * (1 + np.arange(e.B))
    a["T"] = (2.0 + 0.25 * np.arange(e.B * 16)).reshape(e.B, 16)
    return a


PROBLEMS = [("off1", IN(i64, lambda e: e.B)), ("n1", IN(i32, lambda e: e.B)), ("off2", IN(i64, lambda e: e.B)), ("n2", IN(i32, lambda e: e.B))]
LISTS = [("assoc", IN(i32, lambda e: 2 * _n_assoc(e))), ("assoc_off", IN(i64, lambda e: e.B + 1))]
LISTS_DEV = [("assoc", DEV), ("assoc_off", IN(i64, lambda e: e.B + 1))]
SOLVER_OUT = [("kmax", I),
              ("assoc_out", OUT(i32, lambda e: e.B * e.kmax * 2, lambda e: 100 + np.arange(e.B * e.kmax * 2))),
              ("n_assoc_out", OUT(i32, lambda e: e.B, lambda e: _counts(e.B, e.kmax))),
              ("T_out", OUT(f64, lambda e: e.B * 16, lambda e: 1.0 + 0.5 * np.arange(e.B * 16))),
              ("status_out", OUT(i32, lambda e: e.B, lambda e: 3 + np.arange(e.B))),
              ("stats_out", OUT(rt.stats_dtype(), lambda e: e.B, lambda e: _fill_stats(e, e.B)))]
SOLVER_OUT_DEV = [("kmax", I), ("assoc_out", DEV), ("n_assoc_out", DEV), ("T_out", DEV), ("status_out", DEV), ("stats_out", DEV)]
MNO_OUT = [("num_solutions", I), ("kmax", I),
           ("assoc_out", OUT(i32, lambda e: e.B * e.Kc * e.kmax * 2, lambda e: 100 + np.arange(e.B * e.Kc * e.kmax * 2))),
           ("sol_out", OUT(rt.mno_solution_dtype(), lambda e: e.B * e.Kc, _fill_sol)),
           ("stats_out", OUT(rt.stats_dtype(), lambda e: e.B * e.Kc, lambda e: _fill_stats(e, e.B * e.Kc)))]
MNO_OUT_DEV = [("num_solutions", I), ("kmax", I), ("assoc_out", DEV), ("sol_out", DEV), ("stats_out", DEV)]
RANSAC_OUT = [("kmax", I),
              ("assoc_out", OUT(i32, lambda e: e.B * e.kmax * 2, lambda e: 100 + np.arange(e.B * e.kmax * 2))),
              ("rec_out", OUT(rt.ransac_record_dtype(), lambda e: e.B, _fill_ransac)),
              ("counts_out", OUT(i32, lambda e: e.B * max(int(e.ref("rparams").max_iteration), 0),
                                 lambda e: 50 + np.arange(e.B * max(int(e.ref("rparams").max_iteration), 0))))]
RANSAC_SPLIT = [("T_out", OUT(f64, lambda e: e.B * 16, lambda e: 1.0 + 0.5 * np.arange(e.B * 16))),
                ("n_assoc_out", OUT(i32, lambda e: e.B, lambda e: _counts(e.B, e.kmax))),
                ("status_out", OUT(i32, lambda e: e.B, lambda e: 3 + np.arange(e.B)))]
LC_IN = [("lc_params", REF), ("T_ref", IN(f64, lambda e: e.B * 16)), ("enable", IN(i32, lambda e: e.B)),
         ("FL", IN(f64, lambda e: e.n_left * 16)), ("n_left", I), ("iL", IN(i32, lambda e: e.B)),
         ("FR", IN(f64, lambda e: e.n_right * 16)), ("n_right", I), ("iR", IN(i32, lambda e: e.B))]
LC_IN_DEV = [("lc_params", REF), ("T_ref", DEV), ("enable", DEV), ("FL", DEV), ("iL", DEV), ("FR", DEV), ("iR", DEV)]
TAIL_OUT = [("records", OUT(rt.lc_record_dtype(), lambda e: e.B, lambda e: _fill_lc_records(e, e.B))),
            ("accepted_idx", OUT(i32, lambda e: max(e.B, 1), lambda e: 7 + np.arange(max(e.B, 1)))),
            ("n_accepted", OUT(i32, lambda e: 1, lambda e: [max(e.B - 1, 0)]))]
TAIL_OUT_DEV = [("records", DEV), ("accepted_idx", DEV), ("n_accepted", DEV)]
MNO_TAIL_OUT = [("records", OUT(rt.lc_record_dtype(), lambda e: e.B * e.Kc, lambda e: _fill_lc_records(e, e.B * e.Kc))),
                ("best", OUT(i32, lambda e: max(e.B, 1), lambda e: np.arange(max(e.B, 1)) - 1)),
                ("accepted_idx", OUT(i32, lambda e: max(e.B * e.Kc, 1), lambda e: 7 + np.arange(max(e.B * e.Kc, 1)))),
                ("n_accepted", OUT(i32, lambda e: 1, lambda e: [max(e.B * e.Kc - 1, 0)])),
                ("accepted_best_idx", OUT(i32, lambda e: max(e.B, 1), lambda e: 9 + np.arange(max(e.B, 1)))),
                ("n_accepted_best", OUT(i32, lambda e: 1, lambda e: [max(e.B - 1, 0)]))]
MNO_TAIL_OUT_DEV = [("records", DEV), ("best", DEV), ("accepted_idx", DEV), ("n_accepted", DEV), ("accepted_best_idx", DEV), ("n_accepted_best", DEV)]
HEAD = [("ctx", H), ("params", REF), ("B", I)]
RHEAD = [("ctx", H), ("rparams", REF), ("B", I)]
POOL = [("feats", IN(f64, lambda e: e.n_objects * e.F)), ("n_objects", I)]
U0 = [("u0", IN(f64, _n_assoc))]
_rows = lambda e: int(e.arr("n1").sum(dtype=np.int64) + e.arr("n2").sum(dtype=np.int64))

ENTRIES = {
    "roman_align_batch": HEAD + POOL + PROBLEMS + [("F", I)] + LISTS + U0 + SOLVER_OUT,
    "roman_align_batch_resident": HEAD + [("feats", DEV)] + PROBLEMS + [("F", I)] + LISTS_DEV + [("u0", DEV)] + SOLVER_OUT,
    "roman_align_batch_dev": HEAD + [("feats", DEV)] + PROBLEMS + [("F", I)] + LISTS_DEV + [("u0", DEV)] + SOLVER_OUT_DEV,
    "roman_align_lc_batch": HEAD + POOL + PROBLEMS + [("F", I)] + LISTS + U0 + SOLVER_OUT + LC_IN + TAIL_OUT,
    "roman_align_lc_batch_ids": HEAD + POOL + PROBLEMS + [("F", I)] + LISTS + U0 + SOLVER_OUT + LC_IN + TAIL_OUT + [
        ("ids", IN(i64, lambda e: e.n_objects)),
        ("n1_kept", OUT(i32, lambda e: e.B, lambda e: np.maximum(e.arr("n1") - 1, 0))),
        ("n2_kept", OUT(i32, lambda e: e.B, lambda e: e.arr("n2"))),
        ("keep", OUT(i32, _rows, lambda e: 60 + np.arange(_rows(e))))],
    "roman_align_lc_batch_dev": HEAD + [("feats", DEV)] + PROBLEMS + [("F", I)] + LISTS_DEV + [("u0", DEV)] + SOLVER_OUT_DEV + LC_IN_DEV + TAIL_OUT_DEV,
    "roman_lc_tail_dev": [("ctx", H), ("lc_params", REF), ("B", I), ("T", DEV), ("n_assoc", DEV), ("status", DEV)] + LC_IN_DEV[1:] + TAIL_OUT_DEV,
    "roman_mno_batch": HEAD + POOL + PROBLEMS + [("F", I)] + LISTS + MNO_OUT,
    "roman_mno_batch_dev": HEAD + [("feats", DEV)] + PROBLEMS + [("F", I)] + LISTS_DEV + MNO_OUT_DEV,
    "roman_mno_lc_batch": HEAD + POOL + PROBLEMS + [("F", I)] + LISTS + MNO_OUT + LC_IN + MNO_TAIL_OUT,
    "roman_mno_lc_batch_dev": HEAD + [("feats", DEV)] + PROBLEMS + [("F", I)] + LISTS_DEV + MNO_OUT_DEV + LC_IN_DEV + MNO_TAIL_OUT_DEV,
    "roman_mno_lc_tail_dev": [("ctx", H), ("lc_params", REF), ("B", I), ("K", I), ("sol", DEV)] + LC_IN_DEV[1:] + MNO_TAIL_OUT_DEV,
    "roman_ransac_batch": RHEAD + [("pts", IN(f64, lambda e: e.n_objects * 3)), ("n_objects", I)] + PROBLEMS + RANSAC_OUT,
    "roman_ransac_batch_dev": RHEAD + [("pts", DEV)] + PROBLEMS + [("kmax", I), ("assoc_out", DEV), ("rec_out", DEV), ("counts_out", DEV)],
    "roman_ransac_lc_batch": RHEAD + [("rows", IN(f64, lambda e: e.n_objects * e.F)), ("n_objects", I), ("F", I)] + PROBLEMS + RANSAC_OUT + RANSAC_SPLIT
                             + LC_IN + TAIL_OUT,
    "roman_ransac_lc_batch_dev": RHEAD + [("rows", DEV), ("F", I)] + PROBLEMS + [("kmax", I), ("assoc_out", DEV), ("rec_out", DEV), ("counts_out", DEV),
                                                                                 ("T_out", DEV), ("n_assoc_out", DEV), ("status_out", DEV)]
                                 + LC_IN_DEV + TAIL_OUT_DEV,
    "roman_shared_ids_dev": [("ctx", H), ("B", I), ("ids", DEV)] + PROBLEMS + [("keep", DEV), ("kept", DEV)],
    "roman_shared_reduce_dev": [("ctx", H), ("B", I), ("F", I), ("feats", DEV), ("region_row0", I), ("ids", DEV)] + PROBLEMS + [("keep", DEV), ("kept", DEV)],
}
# host outputs whose contents on entry are not defined (roman_align_batch_resident writes every one of them before it returns 0 or
# ROMAN_E_INTERNAL): what the wrapper returns after the recorder has filled them is compared, not what they held when handed in
UNDEFINED_ON_ENTRY = {"roman_align_batch_resident": {"assoc_out", "n_assoc_out", "T_out", "status_out", "stats_out"}}


RECORD_NAMES = {rt.stats_dtype(): "roman_stats_t", rt.lc_record_dtype(): "roman_lc_record_t", rt.mno_solution_dtype(): "roman_mno_solution_t",
                rt.ransac_record_dtype(): "roman_ransac_record_t"}


def encode(a):
    """An array as plain data, exactly: the values of a plain dtype, of a record dtype field by field (its padding is nobody's);
    an array of one repeated value (a cleared output block) as that value."""
    a = np.asarray(a)
    d = {"dtype": RECORD_NAMES.get(a.dtype, str(a.dtype)), "shape": list(a.shape)}
    if a.dtype.fields is not None:
        if a.size > 1 and not any(np.any(a[f]) for f in a.dtype.names):
            d["every"] = 0
        else:
            d["fields"] = {f: a[f].ravel().tolist() for f in a.dtype.names}
    elif a.size > 1 and (a == a.ravel()[0]).all():
        d["every"] = a.ravel()[0].item()
    else:
        d["values"] = a.ravel().tolist()
    return d


class _Env:
    def __init__(self, spec, args):
        self.kind = dict(spec)
        self.raw = {name: a for (name, _), a in zip(spec, args)}

    def given(self, name):
        return self.raw[name] is not None

    def ref(self, name):
        return self.raw[name]._obj

    def arr(self, name):
        _, dtype, count = self.kind[name][:3]
        return _arr(self.raw[name], int(count(self)), dtype)

    @property
    def Kc(self):
        return max(self.raw.get("num_solutions", self.raw.get("K")), 0)

    def __getattr__(self, name):                                   # the call's integers by name
        raw = self.__dict__["raw"]
        if name in raw and self.__dict__["kind"][name] == I:
            return raw[name]
        raise AttributeError(name)


class CallRecorder(RecordingLib):
    """Every entry of ENTRIES: log the name, decode the arguments into `transcript`, fill the host outputs, return `rc`."""

    def __init__(self):
        super().__init__(None)
        self.rc = 0
        self.transcript = []
        self.out_addr = {}                                         # of the latest call: host output name -> address

    def roman_last_error(self, h):
        return LAST_ERROR

    def __getattr__(self, name):
        if name in ENTRIES:
            return lambda *a: self._entry(name, a)
        return super().__getattr__(name)

    def _entry(self, name, args):
        spec = ENTRIES[name]
        self._log(name)
        assert len(args) == len(spec), f"{name}: {len(args)} arguments, the header has {len(spec)}"
        e = _Env(spec, args)
        decoded, self.out_addr = [], {}
        for (arg, kind), a in zip(spec, args):
            if kind == I:
                assert type(a) is int, f"{name}.{arg}: {type(a).__name__} where the ABI takes an integer"
                v = a
            elif kind in (H, DEV):
                assert a is None or type(a).__name__ == "c_void_p", f"{name}.{arg}: {type(a).__name__} where the ABI takes an address"
                v = None if a is None else a.value
            elif kind == REF:
                assert a is None or hasattr(a, "_obj"), f"{name}.{arg}: {type(a).__name__} where the ABI takes a byref structure"
                v = None if a is None else {"struct": type(a._obj).__name__, "hex": bytes(a._obj).hex()}
            elif a is None:
                v = None
            else:
                assert type(a).__name__ == "c_void_p", f"{name}.{arg}: {type(a).__name__} where the ABI takes a host pointer"
                if kind[0] == "out":
                    self.out_addr[arg] = a.value
                if kind[0] == "out" and arg in UNDEFINED_ON_ENTRY.get(name, ()):
                    v = {"dtype": RECORD_NAMES.get(np.dtype(kind[1]), str(np.dtype(kind[1]))), "count": int(kind[2](e)), "on_entry": "undefined"}
                else:
                    v = encode(e.arr(arg))
            decoded.append([arg, v])
        for (arg, kind), a in zip(spec, args):                     # the outputs, once everything handed in has been read
            if isinstance(kind, tuple) and kind[0] == "out" and a is not None:
                values = np.ascontiguousarray(kind[3](e), dtype=kind[1])
                assert values.size == int(kind[2](e))
                _put(a, values, kind[1])
        self.transcript.append({"entry": name, "args": decoded})
        return self.rc


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (tiny: B <= 3, n <= 4, F <= 5, K <= 2) — of the wrong dtype and kind on purpose, so that the binding must convert them
# ---------------------------------------------------------------------------------------------------------------------------
def params(dim=3):
    P = _abi.RomanParams.default()
    P.point_dim = dim
    return P


def rparams(max_iteration=4):
    R = _abi.RomanRansacParams()
    R.max_iteration = max_iteration; R.round = 2; R.edge_len = 0.9; R.max_dist = 0.25; R.confidence = 0.999; R.seed = 1234567
    return R


def pool(n, F, as_list=False):
    a = (0.25 * np.arange(n * F)).reshape(n, F).astype(np.float32)
    return a.tolist() if as_list else a


P0 = dict(off1=[], n1=[], off2=[], n2=[])                                                          # B = 0; n_objects 0
P1 = dict(off1=[0], n1=[0], off2=[0], n2=[0])                                                      # one problem of two empty maps
P2 = dict(off1=np.array([0, 7], dtype=np.int32), n1=np.array([4, 2], dtype=np.int64), off2=[4, 9], n2=[3, 1])      # 10 objects
P3 = dict(off1=[0, 7, 9], n1=[4, 0, 2], off2=[4, 7, 11], n2=np.array([3, 2, 1], dtype=np.int16))   # 12 objects, problem 1 has an empty map
NOBJ = {0: 0, 1: 0, 2: 10, 3: 12}
ASSOC2 = dict(assoc=np.array([[0, 0], [1, 2], [3, 1]], dtype=np.int64), assoc_off=np.array([0, 3, 3], dtype=np.int32))    # problem 1: an empty list
DEVP = {k: 0x1000 * (i + 1) for i, k in enumerate(
    ["feats", "assoc_out", "n_out", "T_out", "status", "stats", "assoc", "u0", "records", "idx", "cnt", "T_ref", "enable", "FL", "iL", "FR", "iR",
     "sol", "best", "bidx", "bcnt", "rec", "counts", "ids", "keep", "kept"])}
LC_DEV_ALL = dict(T_ref_ptr=DEVP["T_ref"], enable_ptr=DEVP["enable"], FL_ptr=DEVP["FL"], iL_ptr=DEVP["iL"], FR_ptr=DEVP["FR"], iR_ptr=DEVP["iR"])


def frames(S, base):
    return (base + 0.5 * np.arange(S * 16)).reshape(S, 4, 4).astype(np.float32)


def lc_inputs(kind, B):
    """LcInputs: 'none', 'ref' (T_ref + enable), 'left' (FL + iL), 'both' (everything; S0 = 3, S1 = 2), 'orphan' (FL without iL)."""
    kw = {}
    if kind in ("ref", "both"):
        kw.update(T_ref=frames(B, 1.0).tolist(), enable=[b % 2 for b in range(B)])
    if kind in ("left", "both", "orphan"):
        kw.update(FL=frames(3, 2.0))
    if kind in ("left", "both"):
        kw.update(iL=np.arange(B, dtype=np.int64) % 3)
    if kind == "both":
        kw.update(FR=frames(2, 3.0).tolist(), iR=[b % 2 for b in range(B)], tilt_thresh=0.3, force_rm_upside_down=True, lc_association_thresh=5)
    return rt.LcInputs(**kw)


def _cases():
    """-> [(id, method, args, kwargs, rc)].  Arguments are built afresh on every call of this function."""
    out = []

    def case(cid, method, *args, rc=0, **kw):
        out.append((cid, method, args, kw, rc))

    def rcs(cid, method, *args, **kw):                             # the same call at rc = 0, ROMAN_E_INTERNAL and another code
        case(cid, method, *args, **kw)
        case(cid + "-internal", method, *args, rc=_abi.ROMAN_E_INTERNAL, **kw)
        case(cid + "-toolarge", method, *args, rc=_abi.ROMAN_E_TOO_LARGE, **kw)

    tab = lambda P: (P["off1"], P["n1"], P["off2"], P["n2"])
    u0 = [0.5, 0.25, 0.125]
    # ---- align
    rcs("align_batch/B2", "align_batch", params(), pool(10, 5), *tab(P2))
    case("align_batch/B0", "align_batch", params(), np.zeros((0, 5)), *tab(P0))
    case("align_batch/B2-assoc-u0-kmax", "align_batch", params(), pool(10, 5, as_list=True), *tab(P2), u0=u0, kmax=2, **ASSOC2)
    case("align_batch/B3-empty-map", "align_batch", params(), pool(12, 4), *tab(P3))
    case("align_batch/B1-all-empty", "align_batch", params(), np.zeros((0, 5)), *tab(P1))
    case("align_batch/B2-dim2", "align_batch", params(2), pool(10, 5), *tab(P2))
    case("align_batch/feats-1d", "align_batch", params(), np.zeros(10), *tab(P2))
    rcs("align_batch_resident/B2", "align_batch_resident", params(), DEVP["feats"], 5, *tab(P2))
    case("align_batch_resident/B0", "align_batch_resident", params(), None, 5, *tab(P0))
    case("align_batch_resident/B2-assoc-u0-kmax", "align_batch_resident", params(), DEVP["feats"], np.int64(5), *tab(P2), kmax=np.int32(2),
         assoc_ptr=DEVP["assoc"], assoc_off=[0, 3, 3], u0_ptr=DEVP["u0"])
    case("align_batch_resident/B3-empty-map-dim2", "align_batch_resident", params(2), DEVP["feats"], 4, *tab(P3))
    dev_out = (DEVP["assoc_out"], DEVP["n_out"], DEVP["T_out"], DEVP["status"])
    rcs("align_batch_dev/B2", "align_batch_dev", params(), DEVP["feats"], 5, *tab(P2), 3, *dev_out)
    case("align_batch_dev/B0", "align_batch_dev", params(), 0, 5, *tab(P0), 1, *dev_out)
    case("align_batch_dev/B2-all", "align_batch_dev", params(), DEVP["feats"], np.int64(5), *tab(P2), np.int64(3), *dev_out, stats_out_ptr=DEVP["stats"],
         assoc_ptr=DEVP["assoc"], assoc_off=[0, 3, 3], u0_ptr=DEVP["u0"])
    # ---- loop closures
    rcs("align_lc_batch/B2", "align_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("none", 2))
    case("align_lc_batch/B0", "align_lc_batch", params(), np.zeros((0, 5)), *tab(P0), lc_inputs("none", 0))
    case("align_lc_batch/B2-ref", "align_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("ref", 2), u0=u0, kmax=2, **ASSOC2)
    case("align_lc_batch/B3-left", "align_lc_batch", params(), pool(12, 4), *tab(P3), lc_inputs("left", 3))
    case("align_lc_batch/B3-both", "align_lc_batch", params(), pool(12, 4, as_list=True), *tab(P3), lc_inputs("both", 3))
    case("align_lc_batch/B2-orphan-frames", "align_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("orphan", 2))
    case("align_lc_batch/feats-3d", "align_lc_batch", params(), np.zeros((2, 5, 1)), *tab(P2), lc_inputs("none", 2))
    ids10, ids12 = [100 + k % 6 for k in range(10)], np.arange(12, dtype=np.int32)
    rcs("align_lc_batch_ids/B2", "align_lc_batch_ids", params(), pool(10, 5), ids10, *tab(P2), lc_inputs("ref", 2))
    case("align_lc_batch_ids/B0", "align_lc_batch_ids", params(), np.zeros((0, 5)), [], *tab(P0), lc_inputs("none", 0))
    case("align_lc_batch_ids/B3-no-keep", "align_lc_batch_ids", params(), pool(12, 4), ids12, *tab(P3), lc_inputs("both", 3), want_keep=False)
    case("align_lc_batch_ids/B2-u0-kmax", "align_lc_batch_ids", params(), pool(10, 5), ids10, *tab(P2), lc_inputs("left", 2), u0=np.ones(14, dtype=np.float32), kmax=4)
    case("align_lc_batch_ids/ids-length", "align_lc_batch_ids", params(), pool(10, 5), ids10[:9], *tab(P2), lc_inputs("none", 2))
    case("align_lc_batch_ids/feats-1d", "align_lc_batch_ids", params(), np.zeros(10), ids10, *tab(P2), lc_inputs("none", 2))
    case("align_lc_batch_ids/B2-orphan-frames", "align_lc_batch_ids", params(), pool(10, 5), ids10, *tab(P2), lc_inputs("orphan", 2))
    lp = lc_inputs("both", 2).params()
    tail_out = (DEVP["records"], DEVP["idx"], DEVP["cnt"])
    rcs("align_lc_batch_dev/B2", "align_lc_batch_dev", params(), DEVP["feats"], 5, *tab(P2), 3, *dev_out, lp, *tail_out)
    case("align_lc_batch_dev/B3-all", "align_lc_batch_dev", params(), DEVP["feats"], 4, *tab(P3), np.int64(3), *dev_out, lp, *tail_out, stats_out_ptr=DEVP["stats"],
         assoc_ptr=DEVP["assoc"], assoc_off=np.array([0, 3, 3, 5], dtype=np.int32), u0_ptr=DEVP["u0"], **LC_DEV_ALL)
    case("align_lc_batch_dev/B0", "align_lc_batch_dev", params(), None, 5, *tab(P0), 1, None, None, None, None, lc_inputs("none", 0).params(), None, None, None)
    rcs("lc_tail_dev/B2", "lc_tail_dev", lp, 2, DEVP["T_out"], DEVP["n_out"], DEVP["status"], *tail_out)
    case("lc_tail_dev/B3-all", "lc_tail_dev", lp, np.int64(3), DEVP["T_out"], DEVP["n_out"], DEVP["status"], *tail_out, **LC_DEV_ALL)
    case("lc_tail_dev/B0", "lc_tail_dev", lc_inputs("none", 0).params(), 0, None, None, None, None, None, None)
    # ---- multi-hypothesis
    rcs("mno_batch/B2-K2", "mno_batch", params(), pool(10, 5), *tab(P2))
    case("mno_batch/B0", "mno_batch", params(), np.zeros((0, 5)), *tab(P0))
    case("mno_batch/B2-K0", "mno_batch", params(), pool(10, 5), *tab(P2), num_solutions=0)
    case("mno_batch/B2-K1-assoc-kmax", "mno_batch", params(), pool(10, 5, as_list=True), *tab(P2), num_solutions=np.int64(1), kmax=2, **ASSOC2)
    case("mno_batch/B3-empty-map-dim2", "mno_batch", params(2), pool(12, 4), *tab(P3))
    case("mno_batch/feats-1d", "mno_batch", params(), np.zeros(10), *tab(P2))
    mno_out = (DEVP["assoc_out"], DEVP["sol"])
    rcs("mno_batch_dev/B2", "mno_batch_dev", params(), DEVP["feats"], 5, *tab(P2), 2, 3, *mno_out)
    case("mno_batch_dev/B3-all", "mno_batch_dev", params(), DEVP["feats"], np.int64(4), *tab(P3), np.int64(2), np.int64(3), *mno_out, stats_out_ptr=DEVP["stats"],
         assoc_ptr=DEVP["assoc"], assoc_off=[0, 3, 3, 5])
    case("mno_batch_dev/B0", "mno_batch_dev", params(), None, 5, *tab(P0), 2, 1, None, None)
    rcs("mno_lc_batch/B2-K2", "mno_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("both", 2))
    case("mno_lc_batch/B0", "mno_lc_batch", params(), np.zeros((0, 5)), *tab(P0), lc_inputs("none", 0))
    case("mno_lc_batch/B2-K0", "mno_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("ref", 2), num_solutions=0)
    case("mno_lc_batch/B3-K1-assoc-kmax", "mno_lc_batch", params(), pool(12, 4, as_list=True), *tab(P3), lc_inputs("left", 3), num_solutions=1, kmax=2,
         assoc=[[0, 0], [1, 2], [3, 1], [0, 0], [1, 0]], assoc_off=[0, 3, 3, 5])
    case("mno_lc_batch/B3-empty-map-dim2", "mno_lc_batch", params(2), pool(12, 4), *tab(P3), lc_inputs("none", 3))
    case("mno_lc_batch/B2-orphan-frames", "mno_lc_batch", params(), pool(10, 5), *tab(P2), lc_inputs("orphan", 2))
    case("mno_lc_batch/feats-1d", "mno_lc_batch", params(), np.zeros(10), *tab(P2), lc_inputs("none", 2))
    mno_tail_out = (DEVP["records"], DEVP["best"], DEVP["idx"], DEVP["cnt"], DEVP["bidx"], DEVP["bcnt"])
    rcs("mno_lc_batch_dev/B2", "mno_lc_batch_dev", params(), DEVP["feats"], 5, *tab(P2), 2, 3, *mno_out, lp, *mno_tail_out)
    case("mno_lc_batch_dev/B3-all", "mno_lc_batch_dev", params(), DEVP["feats"], 4, *tab(P3), 2, np.int64(3), *mno_out, lp, *mno_tail_out, stats_out_ptr=DEVP["stats"],
         assoc_ptr=DEVP["assoc"], assoc_off=[0, 3, 3, 5], **LC_DEV_ALL)
    case("mno_lc_batch_dev/B0", "mno_lc_batch_dev", params(), None, 5, *tab(P0), 2, 1, None, None, lc_inputs("none", 0).params(), *[None] * 6)
    rcs("mno_lc_tail_dev/B2", "mno_lc_tail_dev", lp, 2, 2, DEVP["sol"], *mno_tail_out)
    case("mno_lc_tail_dev/B3-all", "mno_lc_tail_dev", lp, np.int64(3), np.int64(1), DEVP["sol"], *mno_tail_out, **LC_DEV_ALL)
    # ---- RANSAC
    rcs("ransac_batch/B2", "ransac_batch", rparams(), pool(10, 3), *tab(P2))
    case("ransac_batch/B0", "ransac_batch", rparams(), np.zeros((0, 3)), *tab(P0), counts=True)
    case("ransac_batch/B3-empty-map-counts", "ransac_batch", rparams(), pool(12, 3, as_list=True), *tab(P3), counts=True)
    case("ransac_batch/B1-all-empty", "ransac_batch", rparams(), np.zeros((0, 3)), *tab(P1))
    case("ransac_batch/B2-kmax-own-counts", "ransac_batch", rparams(), pool(10, 3), *tab(P2), kmax=5, counts=np.full((2, 4), -9, dtype=np.int32))
    case("ransac_batch/counts-dtype", "ransac_batch", rparams(), pool(10, 3), *tab(P2), counts=np.zeros((2, 4), dtype=np.int64))
    case("ransac_batch/counts-shape", "ransac_batch", rparams(), pool(10, 3), *tab(P2), counts=np.zeros((2, 5), dtype=np.int32))
    case("ransac_batch/counts-strided", "ransac_batch", rparams(), pool(10, 3), *tab(P2), counts=np.zeros((2, 8), dtype=np.int32)[:, ::2])
    case("ransac_batch/pts-width", "ransac_batch", rparams(), pool(10, 4), *tab(P2))
    rcs("ransac_batch_dev/B2", "ransac_batch_dev", rparams(), DEVP["feats"], *tab(P2), 12, DEVP["assoc_out"], DEVP["rec"])
    case("ransac_batch_dev/B3-counts", "ransac_batch_dev", rparams(), DEVP["feats"], *tab(P3), np.int64(12), DEVP["assoc_out"], DEVP["rec"], counts_out_ptr=DEVP["counts"])
    case("ransac_batch_dev/B0", "ransac_batch_dev", rparams(), None, *tab(P0), 1, None, None)
    rcs("ransac_lc_batch/B2", "ransac_lc_batch", rparams(), pool(10, 5), *tab(P2), lc_inputs("ref", 2))
    case("ransac_lc_batch/B0", "ransac_lc_batch", rparams(), np.zeros((0, 3)), *tab(P0), lc_inputs("none", 0))
    case("ransac_lc_batch/B3-both-counts", "ransac_lc_batch", rparams(), pool(12, 4, as_list=True), *tab(P3), lc_inputs("both", 3), counts=True)
    case("ransac_lc_batch/B2-kmax-own-counts", "ransac_lc_batch", rparams(), pool(10, 3), *tab(P2), lc_inputs("left", 2), kmax=5, counts=np.full((2, 4), -9, dtype=np.int32))
    case("ransac_lc_batch/B1-all-empty", "ransac_lc_batch", rparams(), np.zeros((0, 3)), *tab(P1), lc_inputs("none", 1))
    case("ransac_lc_batch/counts-dtype", "ransac_lc_batch", rparams(), pool(10, 5), *tab(P2), lc_inputs("none", 2), counts=np.zeros((2, 4), dtype=np.int64))
    case("ransac_lc_batch/counts-shape", "ransac_lc_batch", rparams(), pool(10, 5), *tab(P2), lc_inputs("none", 2), counts=np.zeros((3, 4), dtype=np.int32))
    case("ransac_lc_batch/counts-strided", "ransac_lc_batch", rparams(), pool(10, 5), *tab(P2), lc_inputs("none", 2), counts=np.zeros((4, 4), dtype=np.int32)[::2])
    case("ransac_lc_batch/rows-width", "ransac_lc_batch", rparams(), pool(10, 2), *tab(P2), lc_inputs("none", 2))
    case("ransac_lc_batch/B2-orphan-frames", "ransac_lc_batch", rparams(), pool(10, 5), *tab(P2), lc_inputs("orphan", 2))
    rcs("ransac_lc_batch_dev/B2-no-tail", "ransac_lc_batch_dev", rparams(), DEVP["feats"], 5, *tab(P2), 12, DEVP["assoc_out"], DEVP["rec"])
    case("ransac_lc_batch_dev/B3-all", "ransac_lc_batch_dev", rparams(), DEVP["feats"], np.int64(4), *tab(P3), np.int64(12), DEVP["assoc_out"], DEVP["rec"],
         T_out_ptr=DEVP["T_out"], n_assoc_out_ptr=DEVP["n_out"], status_out_ptr=DEVP["status"], lc_params=lp, records_ptr=DEVP["records"],
         accepted_idx_ptr=DEVP["idx"], n_accepted_ptr=DEVP["cnt"], counts_out_ptr=DEVP["counts"], **LC_DEV_ALL)
    # ---- shared ids
    rcs("shared_ids_dev/B2", "shared_ids_dev", 2, DEVP["ids"], *tab(P2), DEVP["keep"], DEVP["kept"])
    case("shared_ids_dev/B0", "shared_ids_dev", 0, None, *tab(P0), None, None)
    rcs("shared_reduce_dev/B2", "shared_reduce_dev", 2, 5, DEVP["feats"], 10, DEVP["ids"], *tab(P2), DEVP["keep"], DEVP["kept"])
    case("shared_reduce_dev/B3", "shared_reduce_dev", np.int64(3), np.int64(4), DEVP["feats"], np.int64(12), DEVP["ids"], *tab(P3), DEVP["keep"], DEVP["kept"])
    return out


CASE_IDS = [c[0] for c in _cases()]


def _encode_result(res, out_addr):
    """A result dataclass as plain data; every array with `is_output`: the name of the host output it IS (not a copy), or None."""
    names = {addr: name for name, addr in out_addr.items()}

    def enc(v):
        if isinstance(v, np.ndarray):
            d = encode(v)
            d["is_output"] = names.get(v.ctypes.data) if v.size else None
            return d
        if isinstance(v, (list, tuple)):
            return [enc(x) for x in v]
        assert v is None or isinstance(v, (int, float)), type(v)
        return v
    if res is None:
        return None
    return {"class": type(res).__name__, "fields": [[f.name, enc(getattr(res, f.name))] for f in dataclasses.fields(res)]}


def run_case(case):
    """One case against a fresh recorder (install it behind _abi first: see recording()) -> its record."""
    cid, method, args, kw, rc = case
    rec = _abi._LIB
    ctx = rt.Context(0)
    rec.rc, rec.transcript, rec.out_addr = rc, [], {}
    n_calls, gen = len(rec.calls), ctx._generation
    record = {"method": method, "rc": rc}
    try:
        res = getattr(ctx, method)(*args, **kw)
        record["outcome"] = "returned"
        record["result"] = _encode_result(res, rec.out_addr)
        if "counts" in kw and isinstance(kw["counts"], np.ndarray):
            record["callers_counts_after"] = encode(kw["counts"])         # the caller's own array was what the library wrote
            if hasattr(res, "counts"):
                record["counts_is_the_callers"] = res.counts is kw["counts"]
    except (ValueError, rt.RomanHipError) as err:
        record["outcome"] = "raised"
        record["exception"] = {"type": type(err).__name__, "message": str(err), "code": getattr(err, "code", None),
                               "has_result": hasattr(err, "result"), "result": _encode_result(getattr(err, "result", None), rec.out_addr)}
    record["calls"] = rec.calls[n_calls:]
    record["transcript"] = rec.transcript
    record["generation_delta"] = ctx._generation - gen
    rec.rc = 0
    ctx.close()
    return record


def signatures():
    return {m: [[p.name, str(p.kind), None if p.default is inspect.Parameter.empty else repr(p.default)]
                for p in inspect.signature(getattr(rt.Context, m)).parameters.values()] for m in METHODS}


def run_all():
    """Every case -> {"signatures": ..., "cases": {id: record}} (the recorder must stand behind _abi._LIB).  The same call at
    another return code (id + "-internal" / "-toolarge") says {"same_as": id} where its transcript — and the result its error
    carries — equal those of the rc = 0 case: that is what must hold, and the file stays small."""
    cases = {c[0]: run_case(c) for c in _cases()}
    for cid, r in cases.items():
        base = cases.get(cid.rsplit("-", 1)[0]) if cid.endswith(("-internal", "-toolarge")) else None
        if base is None:
            continue
        if r["transcript"] == base["transcript"]:
            r["transcript"] = {"same_as": cid.rsplit("-", 1)[0]}
        if r["exception"]["result"] is not None and r["exception"]["result"] == base["result"]:
            r["exception"]["result"] = {"same_as": cid.rsplit("-", 1)[0]}
    return {"signatures": signatures(), "cases": cases}
