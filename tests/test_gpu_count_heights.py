"""The prefiltered pair tests (k_count, count_rows_pre) take the heights of a candidate's two objects from a per-object table in
LDS (n1 + 1 + n2 doubles per workgroup, indexed like the packed bin table: map-1 objects, the sentinel, map-2 objects) instead
of two gathers from the live pools.  What k_count writes — the mask words and, for whole problems, the rows' degrees (rowCnt) —
is read back through what is built from nothing else: the upper CSR (the decoded words), the stream layout that the degrees
order, and the solver's iterate on it, bit for bit.  Every case runs the prefiltered sweep with the table (row blocks and whole
problems), the prefiltered sweep with the heights from memory (ROMAN_COUNT_ZLDS=0: what a launch without the LDS room takes) and
the plain sweep (ROMAN_COUNT_PRE=0), and compares all of them with the oracle's pattern."""
import numpy as np
import pytest

from conftest import registration_for
from roman_amd import _abi, synth
from roman_amd.align import batch as rb

pytestmark = pytest.mark.gpu

# (ROMAN_COUNT_PRE, ROMAN_COUNT_ZLDS, ROMAN_COUNT_WHOLE): the plain sweep first (the reference of the others)
SWEEPS = [("0", "1", "0"), ("1", "1", "0"), ("1", "1", "1"), ("1", "0", "0"), ("1", "0", "1")]
MODES = [("semanticgrav", 0), ("semanticgrav", 2), ("gravity", 2)]      # (method, gravity_mode: 2 = the z gate)
MODE_IDS = ["semgrav", "semgrav_zgate", "grav_zgate"]


def _reg(method, gmode, d):
    reg = registration_for(method, **({"semantics_dim": d} if method == "semanticgrav" else {}))
    reg._abi_params().gravity_mode = gmode
    return reg


def _nudge(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def _copy(P):
    return type(P).from_buffer_copy(P)


def _all_sweeps(ctx, orc, P, D1, D2, A, monkeypatch):
    """Every sweep's upper CSR is the oracle's (pattern, values, diagonal), its selection the oracle's, and iterate, score and
    counts are the plain sweep's bit for bit.  -> the oracle's (rowptr, cols) over the association list, and the live set's size."""
    mat, Ao = orc.build_matrix(P, D1, D2, A)
    sol = orc.solve(P, mat)
    rp_o, c_o, v_o, d_o = mat.export()
    monkeypatch.setenv("ROMAN_LISTS", "1")
    first = None
    for pre, zlds, whole in SWEEPS:
        monkeypatch.setenv("ROMAN_COUNT_PRE", pre)
        monkeypatch.setenv("ROMAN_COUNT_ZLDS", zlds)
        monkeypatch.setenv("ROMAN_COUNT_WHOLE", whole)
        tag = (pre, zlds, whole)
        ctx.score(P, D1, D2, A)
        rp, cc, vv, dd = ctx.upper_csr()
        assert np.array_equal(rp, rp_o) and np.array_equal(cc, c_o), tag
        assert np.array_equal(vv, v_o) and np.array_equal(dd, d_o), tag
        ctx.solve(None)
        nodes, u, score, st = ctx.solution()
        assert np.array_equal(nodes, sol["nodes"]), tag
        got = (u.copy(), score, (st.n_live, st.nnz_upper, st.n_pass, st.outer_iters, st.inner_iters, st.ls_trials))
        if first is None:
            first = got
        else:
            assert np.array_equal(got[0], first[0]) and got[1] == first[1] and got[2] == first[2], tag
    so = sol["stats"]
    assert first[2][:3] == (so.n_live, so.nnz_upper, so.n_pass)
    return rp_o, c_o, so.n_live


def _pair(reg, n1, n2, d, seed):
    pr = synth.make_pair(n1, n2, d, seed, tilt_deg=1.0)
    return reg.pack(pr.map1), reg.pack(pr.map2)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n1,n2,seed,Lsem", [(5, 5, 903, 3), (9, 70, 902, 201), (257, 6, 903, 473)], ids=["5x5", "9x70", "257x6"])
def test_small_uneven_and_wide_maps(ctx, orc, mode, n1, n2, seed, Lsem, monkeypatch):
    """5 x 5: three live rows behind the semantic gate (one quad, partly filled: its last row duplicated), 25 without it (six quads
    and a row).  9 x 70: the table's map-2 half starts behind the sentinel at entry 10.  257 x 6: more than 256 objects a map,
    the bin table staged by lanes that stride the row."""
    method, gmode = mode
    d = 8 if method == "semanticgrav" else 0
    reg = _reg(method, gmode, d); reg.set_context(ctx)
    P = _copy(reg._abi_params())
    if method == "semanticgrav" and n1 != 5:
        P.cosine_min = 0.2; P.cosine_max = 0.9            # (a wide gate: 201 and 473 live columns; all 630 and 1542 without semantics)
    D1, D2 = _pair(reg, n1, n2, d, seed)
    rp, cc, L = _all_sweeps(ctx, orc, P, D1, D2, None, monkeypatch)
    assert L == (n1 * n2 if method == "gravity" else Lsem)


# live sets of exactly 63, 64, 65 and 129 columns: the cosine gate is set between two neighbouring cosines of the seeded pair
@pytest.mark.parametrize("gmode", [0, 2], ids=["combined", "zgate"])
@pytest.mark.parametrize("K", [63, 64, 65, 129])
def test_live_sets_around_one_and_two_words(ctx, orc, K, gmode, monkeypatch):
    n, d = 24, 32
    reg = _reg("semanticgrav", gmode, d); reg.set_context(ctx)
    D1, D2 = _pair(reg, n, n, d, 910 + K)
    cos = np.sort(np.array([orc.cosine(D1[i, 3:], D2[j, 3:]) for i in range(n) for j in range(n)]))[::-1]
    assert cos[K - 1] > cos[K]                               # the K largest are apart from the rest
    P = _copy(reg._abi_params())
    P.cosine_min = float(cos[K]); P.cosine_max = P.cosine_min + 0.2      # (live: cosine > cosine_min, strict)
    assert int((orc.single_scores(P, D1, D2) > 0).sum()) == K
    rp, cc, L = _all_sweeps(ctx, orc, P, D1, D2, None, monkeypatch)
    assert L == K


def _has(rp, cc, r, c):
    r, c = min(r, c), max(r, c)
    return c in cc[rp[r]:rp[r + 1]]


def test_equal_heights_and_a_pair_on_the_z_gates_threshold(ctx, orc, monkeypatch):
    """Objects 0 and 1 of map 1 have the same height to the bit (their table entries are written by several live columns each, and
    their difference is exactly 0); objects 0 and 1 of map 2 lie 8 m apart like them and 1.5 m apart in height.  The associations
    (0, 0) and (1, 1) are then consistent exactly when the z gate lets dz = 1.5 through (dz < epsilon + sin(5 deg) x 8.14): epsilon
    is moved to the smallest double that does (about 0.79, found with the oracle), one ulp below and one ulp above it."""
    reg = _reg("gravity", 2, 0); reg.set_context(ctx)
    n = 12
    D1, D2 = _pair(reg, n, n, 0, 921)
    D1, D2 = D1.copy(), D2.copy()
    D1[0, :3] = [40.0, 40.0, 1.25]; D1[1, :3] = [48.0, 40.0, 1.25]
    D2[0, :3] = [-40.0, 40.0, 0.5]; D2[1, :3] = [-40.0, 48.0, 2.0]
    D2[2, 2] = D2[0, 2]                                       # equal heights in map 2 as well
    P0 = reg._abi_params()
    ra, rb_ = 0 * n + 0, 1 * n + 1                            # all-to-all, every association live: row = i n2 + j

    def present(eps):
        P = _copy(P0); P.epsilon = eps
        mat, _ = orc.build_matrix(P, D1, D2)
        rp, cc, _, _ = mat.export()
        assert len(rp) - 1 == n * n
        return _has(rp, cc, ra, rb_)

    lo, hi = 0.2, 1.5                                         # |8 - sqrt(64 + 1.5^2)| = 0.14 < 0.2: the length gate is open throughout
    assert not present(lo) and present(hi)
    while _nudge(lo, 1) < hi:                                 # bisection over the doubles' bit patterns
        mid = float(np.array((np.array(lo).view(np.int64) + np.array(hi).view(np.int64)) // 2).view(np.float64))
        if present(mid):
            hi = mid
        else:
            lo = mid
    seen = []
    for k in (-1, 0, 1):
        P = _copy(P0); P.epsilon = _nudge(hi, k)
        rp, cc, L = _all_sweeps(ctx, orc, P, D1, D2, None, monkeypatch)
        assert L == n * n
        seen.append(_has(rp, cc, ra, rb_))
    assert seen == [False, True, True]


def _same_results(a, b, B):
    assert np.array_equal(a.status, b.status)
    for i in range(B):
        assert np.array_equal(a.assoc[i], b.assoc[i]), i
    assert np.array_equal(a.T, b.T, equal_nan=True)
    for f in ("n_live", "nnz_upper", "n_pass", "outer_iters", "inner_iters", "ls_trials", "score"):
        assert np.array_equal(a.stats[f], b.stats[f]), f


@pytest.mark.parametrize("gmode", [0, 2], ids=["combined", "zgate"])
@pytest.mark.parametrize("B", [3, 256], ids=["three_problems", "a_problem_per_compute_unit"])
def test_batches_of_row_blocks_and_of_whole_problems(ctx, orc, B, gmode, monkeypatch):
    """A batch of three problems (work items are blocks of rows: the table is staged per item) and one of 256, a problem per
    compute unit of an MI355X, where the library hands k_count whole problems by itself (staged per problem; the degrees go to
    k_lists).  Maps of different sizes in one call: the table's length is the largest map's, its sentinel sits at each problem's n1."""
    d = 16
    reg = _reg("semanticgrav", gmode, d); reg.set_context(ctx)
    pairs = [synth.make_pair(56 + 4 * (k % 5), 64 - 3 * (k % 4), d, 9300 + k, tilt_deg=1.0) for k in range(B)]
    batch = rb.batch_from_pairs(reg, [(p.map1, p.map2) for p in pairs])
    monkeypatch.setenv("ROMAN_LISTS", "1")
    monkeypatch.delenv("ROMAN_COUNT_WHOLE", raising=False)
    out = {}
    for pre, zlds in (("0", "1"), ("1", "1"), ("1", "0")):
        monkeypatch.setenv("ROMAN_COUNT_PRE", pre)
        monkeypatch.setenv("ROMAN_COUNT_ZLDS", zlds)
        out[pre, zlds] = rb.run_batch(reg, batch, ctx=ctx)
    plain = out["0", "1"]
    _same_results(out["1", "1"], plain, B)
    _same_results(out["1", "0"], plain, B)
    assert (plain.status == _abi.ROMAN_ST_OK).all()
    assert (plain.stats["n_live"] > 128).sum() > B // 2       # (smaller live sets are finished by the demo-scale kernel, not by k_count)
    P = reg._abi_params()
    for k in range(0, B, max(1, B // 8)):
        D1, D2 = reg.pack(pairs[k].map1), reg.pack(pairs[k].map2)
        mat, Ao = orc.build_matrix(P, D1, D2, reg._association_list(pairs[k].map1, pairs[k].map2))
        sol = orc.solve(P, mat)
        assert np.array_equal(plain.assoc[k], Ao[sol["nodes"]]), k
        assert (plain.stats["n_live"][k], plain.stats["nnz_upper"][k]) == (sol["stats"].n_live, sol["stats"].nnz_upper), k
