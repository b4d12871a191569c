"""The whole-device solver k_solve_wide at the worst case of its sums and at the size edge of the half copy's fixed-point scale
(tb = min(49, 62 - bits(L - 1)): 49 at L = 8192, 48 at L = 8193), compared with the oracle in what a sum that is slightly off moves
first: u (1e-9, the bound of test_fixed_point_sums_at_the_stream_solvers_limit for the same quantity) and the score.

Which kernel a case runs — read from roman_hip.hip, the library has no report of it (stats and profile stages do not name a kernel):
* DENSE ENTRY (ctx.set_matrix_data + ctx.solve), n > STREAM_MAXL: roman_set_matrix_data sets `D.wide = 1` and `D.idx16 = 0` ("dense
  problems may carry C flags: 32-bit labels") without reading any switch; enqueue_solve then takes k_solve_wide<uint32_t, false>, the
  PLAIN kernel on the fallback layout with 32-bit labels, one problem on the whole device.  ROMAN_WIDE_UPPER is read but its value is
  and-ed with D.idx16: the dense entry CANNOT be steered onto the half copy.  ROMAN_WIDE_IDX16 is read only where a batch is scored
  (enqueue_score), not here.  ROMAN_WIDE_COMPACT is honoured.  ROMAN_WIDE_TEAMS is read, but one problem makes no team unless forced.
  What the tests can see of this: n_pass == 2 + ls_trials (the rescale pass, the first product, one pass per trial) — the stream
  solver k_solve_up counts one more pass per d update, and every case here reaches the d update at least once.
* HALF COPY (k_solve_wide<uint16_t, true>): only problems scored by the library have 16-bit labels.  The cases use a scored
  'gravity' problem of exactly L live associations (explicit association list) through ctx.score + ctx.solve — whose solution
  exposes u — on ONE TEAM of an XCD's compute units (ROMAN_WIDE_TEAMS = "1") with ROMAN_WIDE_UPPER = "1" (the half copy) and = "0"
  (the plain kernel with 16-bit labels, k_solve_wide<uint16_t, false>, on the same team, as the control).  The team matters: the
  switch only picks the instantiation, and build_upper makes the copy only for a stream of >= 16 steps per wave of the team — one
  problem of 0.8 M pairs on the whole device has a quarter of that and would run <uint16_t, true> over the FULL matrix (the note
  above the scored cases; HALF_COPY_MIN_PAIRS is asserted).  That the copy runs is observed by
  test_the_half_copy_runs_and_drops_what_is_below_its_quantum.  Then the smallest BATCH the library itself gives the half copy:
  two problems of >= 8 000 live associations (teams need >= 2 fallback problems: one team per XCD) through roman_align_batch,
  whose result exposes the associations, the score and the iteration counts, not u.
  A scored matrix cannot be all ones (pairs that share an object are never stored): the worst case of the sums is the dense entry's.
"""
import types

import numpy as np
import pytest

import _wide_sums as ws
from roman_amd import _abi

pytestmark = pytest.mark.gpu
U_TOL = 1e-9


def _params(**kw):
    P = _abi.RomanParams.default(); P.invariant = _abi.ROMAN_INV_EUCLIDEAN
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def _pkey(P):
    return (P.maxiniters, P.maxoliters, P.rescale_u0)


@pytest.fixture(scope="module")
def big():
    """One all-ones n x n array (n = 8193: 537 MB) for M and C of every case, one work array for what is not all ones; the
    oracle's matrices and results, computed once per (matrix, start).  Freed at module end."""
    N = ws.N_EDGE_HI
    h = types.SimpleNamespace(N=N, ones=np.ones((N, N)), work=None, work_key=None, held=None, mats={}, refs={})
    yield h
    h.ones = h.work = None; h.mats.clear(); h.refs.clear()


def _square(A, n):
    """A contiguous n x n VIEW of the array's leading n * n elements (no copy: all ones stay all ones, the work array is filled
    through the same view)."""
    return A.reshape(-1)[:n * n].reshape(n, n)


def _matrices(big, key):
    """(M, C) of the case `key` = (name, n); the work array is rewritten only when the key changes."""
    name, n = key
    if name == "ones":
        o = _square(big.ones, n)
        return o, o
    if big.work is None:
        big.work = np.empty((big.N, big.N))
    W = _square(big.work, n)
    if big.work_key != key:
        if name == "m_2^-20":
            W[:] = 2.0 ** -20; np.fill_diagonal(W, 1.0)
        elif name == "block":
            W[:] = 1.0; ws.plant_block(W, n)
        else:
            ws.random_weights(W, n)
        big.work_key = key
    return (_square(big.ones, n), W) if name == "block" else (W, _square(big.ones, n))


def _solve(ctx, orc, big, key, kind, P=None):
    """The device's and the oracle's solution of the case `key` from the start `kind`; a matrix this module uploaded last (same
    key and parameters; the scored cases reset the note) is not uploaded again."""
    P = P or _params()
    n = key[1]
    if big.held != (key, _pkey(P)):
        M, C = _matrices(big, key)
        ctx.set_matrix_data(P, M, C)
        big.held = (key, _pkey(P))
    u0 = ws.start(kind, n)
    ctx.solve(u0)
    sol = ctx.solution()
    rk = (key, _pkey(P), kind)
    if rk not in big.refs:
        if key not in big.mats:
            big.mats.clear()                                     # (one oracle matrix at a time: 33 M pairs each)
            M, C = _matrices(big, key)
            big.mats[key] = orc.matrix_from_dense(M, C)
        big.refs[rk] = orc.solve(P, big.mats[key], u0)
    return sol, big.refs[rk]


def _compare(n, sol, ref, what, nnz=None):
    nodes, u, score, st = sol
    rs = ref["stats"]
    err = float(np.max(np.abs(u - ref["u"]))) if np.all(np.isfinite(u)) else float("inf")
    print(f"{what}: max |u - u_oracle| {err:.3e}, score {score!r} / oracle {rs.score!r}, passes {st.n_pass} / {rs.n_pass}, "
          f"outer {st.outer_iters} / {rs.outer_iters}, selected {len(nodes)} / {len(ref['nodes'])}")
    assert st.n_live == n and st.nnz_upper == (n * (n - 1) // 2 if nnz is None else nnz)
    assert np.all(np.isfinite(u)) and err <= U_TOL
    assert sorted(nodes.tolist()) == sorted(ref["nodes"].tolist())
    # (the stream test's rule, for the reason written there: F itself only when both sides stopped at the same homotopy step)
    assert round(score) == round(rs.score)
    if st.outer_iters == rs.outer_iters:
        assert abs(score - rs.score) < 1e-6
    return err


@pytest.mark.parametrize("n,kind", [(n, k) for n in ws.DENSE_SIZES for k in ws.WORST_STARTS])
def test_all_ones_matrix_on_the_plain_kernel(ctx, orc, big, n, kind):
    """Case 1, dense entry: k_solve_wide<uint32_t, false>, fallback layout with 32-bit labels (module docstring).  M and C all
    ones: every pair stored at the largest weight, rows of n - 1 entries; n = 3073 is the first size the stream solver refuses,
    8192 | 8193 the edge of the half copy's scale (the plain kernel has no scale: here they are the last full slice | the first row
    of a new one).  The oracle takes 3 passes from every start (tests/_wide_sums.py)."""
    sol, ref = _solve(ctx, orc, big, ("ones", n), kind)
    _compare(n, sol, ref, f"all ones n={n} {kind}")
    st = sol[3]
    assert st.n_pass == 2 + st.ls_trials                        # (not the stream solver's count)


@pytest.mark.parametrize("kind", ws.PLACED_STARTS)
def test_start_vectors_with_the_largest_element_at_either_end_and_far_from_one(ctx, orc, big, kind):
    """Case 3, dense entry, n = 8193 all ones, plain kernel with 32-bit labels.  Neither roman_solve nor solve_last rescales or
    rejects a start vector on the host: with rescale_u0 the kernel's first product is M u0 of the RAW vector.  xmax = 2^-600 and
    2^600 then leave double range in |M u0|^2 on BOTH sides (underflow to 0: u stays M u0 unnormalised, ~6e-175; overflow to inf:
    u = 0): score 0, nothing selected, in the oracle and on the device alike.  For 2^-600 the absolute bound says nothing, so u is
    also held RELATIVELY: sums of n terms in another order differ by at most n 2^-53 of the sum, and the half copy's (c) bound
    (tests/test_wide_sums_cpu.py) is n 2^(e - tb - 1) <= n 2^-48 of a sum that is at least xmax >= 2^(e - 1): n 2^-47 covers both."""
    n = big.N
    sol, ref = _solve(ctx, orc, big, ("ones", n), kind)
    _compare(n, sol, ref, f"all ones n={n} {kind}")
    if kind == "xmax_2^-600":
        assert np.all(ref["u"] > 0.0) and np.max(np.abs(sol[1] - ref["u"]) / ref["u"]) <= n * 2.0 ** -47
    if kind == "xmax_2^600":
        assert not sol[1].any() and len(sol[0]) == 0


def test_tiny_weights_against_full_scale_consistency_sums(ctx, orc, big):
    """Case 2, dense entry, n = 8193, plain kernel with 32-bit labels: M = 2^-20 everywhere, C all ones — the M sums are a
    millionth of the C sums of the same pass.  The iteration is the power method on (1 - 2^-20) I + 2^-20 J, which forgets the
    start at 2^-20 per step: from the twelve-decade start the oracle runs into the cap of 200 inner iterations (202 passes, 25 s on
    the CPU), from all ones it stops after 3 with every u equal — and omega = round(1.008) = 1 of 8193 equal elements is a tie, not
    a selection.  So: the twelve-decade start with maxiniters = 10 (12 oracle passes); u still spans a factor 20 there and the one
    selected element is the start's largest, 0.3 % above the next."""
    n = big.N
    sol, ref = _solve(ctx, orc, big, ("m_2^-20", n), "decades", P=_params(maxiniters=10))
    _compare(n, sol, ref, f"M = 2^-20 n={n}")
    assert ref["stats"].n_pass == 12 and len(ref["nodes"]) == 1


def test_planted_inconsistent_block_runs_the_flagged_entries(ctx, orc, big):
    """Case 2, the converse, dense entry, n = 8193, plain kernel with 32-bit labels: M all ones, C = 0 on the 64 x 64 block rows
    [0, 64) x columns [n - 64, n) and its mirror — 8192 stored weights whose label carries the C flag (bit 31): they count in M x
    and not in C x.  With rescale_u0 the all-ones M wipes out any start and the two sides of the block stay tied for over a
    thousand passes (tests/_wide_sums.py); here rescale_u0 = 0 and the start `block_tilted` decide it at once: 7 oracle passes, the
    row side leaves, 8129 selected with a gap of 1.1e-2 in u at the cut."""
    n = big.N
    sol, ref = _solve(ctx, orc, big, ("block", n), "block_tilted", P=_params(rescale_u0=0))
    _compare(n, sol, ref, f"planted block n={n}")
    nodes = set(sol[0].tolist())
    assert ref["stats"].n_pass == 7 and len(nodes) == n - 64 and not nodes & set(range(64))
    assert sol[3].n_pass == 1 + sol[3].ls_trials                # (no rescale pass; not the stream solver's count)


@pytest.mark.parametrize("n", [ws.N_EDGE_LO, ws.N_EDGE_HI])
def test_random_weights_at_the_scale_edge(ctx, orc, big, n):
    """Case 5, the control, dense entry, plain kernel with 32-bit labels: M uniform in (0, 1], symmetric, C all ones, the
    twelve-decade start: wrong here too means wrong at this size, wrong only on all ones means wrong at the worst case.
    6 oracle passes."""
    sol, ref = _solve(ctx, orc, big, ("random", n), "decades")
    _compare(n, sol, ref, f"random weights n={n}")


def test_compaction_switch_leaves_the_plain_kernels_result_bitwise(ctx, orc, big, monkeypatch):
    """Case 4, dense entry, n = 8193 all ones, twelve-decade start, plain kernel with 32-bit labels, ROMAN_WIDE_COMPACT "0" against
    "0x01FF10".  Bitwise equality holds here because no compaction can happen: every element of every multiplied vector is
    positive (u is uniform after the rescale pass), and a copy is cut only when the window's support has fallen below 255/256 of
    the columns.  (Where one does happen the pieces are cut from the shorter stream and the partial sums group differently —
    k_solve_wide's own comment — so bitwise equality is not promised in general: the scored cases below compare each run with the
    oracle instead.)"""
    n = big.N
    out = []
    for compact in ("0", "0x01FF10"):
        monkeypatch.setenv("ROMAN_WIDE_COMPACT", compact)
        sol, ref = _solve(ctx, orc, big, ("ones", n), "decades")
        _compare(n, sol, ref, f"all ones n={n} compaction {compact}")
        out.append(sol)
    (n0, u0, s0, st0), (n1, u1, s1, st1) = out
    assert np.array_equal(u0, u1) and np.array_equal(n0, n1) and s0 == s1 and st0.outer_iters == st1.outer_iters


# ---- the half copy: scored problems (16-bit labels) ------------------------------------------------------------------------------
# build_upper (k_solve_wide) makes the copy only when the full stream has at least 16 steps per wave of the TEAM
# (`Tfull < 16 * NWG` returns before upOn is set; Tfull = nnzCap >> 8, a step = 256 entry slots).  One problem on the whole
# device is a "team" of all 256 compute units x 8 waves: 32 768 steps, 4.2 M stored pairs — the 0.8 M pairs of these problems are
# a quarter of that, and ROMAN_WIDE_UPPER = "1" alone would stream the full matrix in the <uint16_t, true> instantiation.  So the
# single problem is given ONE TEAM PER XCD (ROMAN_WIDE_TEAMS = "1": enqueue_solve accepts a forced team for one fallback problem):
# 32 compute units, NWG = 256, 4096 steps.  nnzCap holds both triangles, so 2 * nnz_upper / 256 >= 4096 suffices:
HALF_COPY_MIN_PAIRS = 16 * (32 * 8) * 256 // 2                  # 524 288 stored pairs; asserted wherever a case claims the half copy


@pytest.fixture(scope="module")
def scored(orc):
    """The two scored problems (L = 8192 | 8193) and the oracle's solutions per start, computed once."""
    probs = {L: ws.gravity_problem(L) for L in (ws.N_EDGE_LO, ws.N_EDGE_HI)}
    refs = {}

    def ref(L, kind):
        if (L, kind) not in refs:
            reg, D1, D2, A = probs[L]
            refs[(L, kind)] = orc.register(reg._abi_params(), D1, D2, A=A, u0=ws.start(kind, L), faithful=False)
        return refs[(L, kind)]
    yield types.SimpleNamespace(probs=probs, ref=ref)
    refs.clear(); probs.clear()


def _scored_solve(ctx, big, scored, L, u0, P=None):
    reg, D1, D2, A = scored.probs[L]
    big.held = None                                              # (the context's dense matrix is gone)
    ctx.score(P or reg._abi_params(), D1, D2, A)
    ctx.solve(u0)
    nodes, u, score, st = ctx.solution()
    return ctx.selected_associations(), u, score, st


def _compare_scored(L, got, o, what):
    assoc, u, score, st = got
    rs = o["stats"]
    err = float(np.max(np.abs(u - o["u"]))) if np.all(np.isfinite(u)) else float("inf")
    print(f"{what}: max |u - u_oracle| {err:.3e}, score {score!r} / oracle {rs.score!r}, passes {st.n_pass} / {rs.n_pass}, "
          f"outer {st.outer_iters} / {rs.outer_iters}, selected {len(assoc)} / {len(o['assoc'])}, stored pairs {st.nnz_upper}")
    assert st.n_live == L == rs.n_live and st.nnz_upper == rs.nnz_upper >= HALF_COPY_MIN_PAIRS
    assert np.all(np.isfinite(u)) and err <= U_TOL
    assert sorted(map(tuple, assoc.tolist())) == sorted(map(tuple, o["assoc"].tolist()))
    assert round(score) == round(rs.score)
    if st.outer_iters == rs.outer_iters:
        assert abs(score - rs.score) < 1e-6
    return err


def _one_team(monkeypatch, upper):
    monkeypatch.setenv("ROMAN_WIDE_TEAMS", "1")
    monkeypatch.setenv("ROMAN_WIDE_UPPER", upper)


@pytest.mark.parametrize("L", [ws.N_EDGE_LO, ws.N_EDGE_HI])
def test_the_half_copy_runs_and_drops_what_is_below_its_quantum(ctx, orc, big, scored, L, monkeypatch):
    """That the cases below really take the copy is OBSERVED, not only read: its pushed terms are integers rint(v x_p 2^(tb - e)).
    Start: 2^-60 everywhere, one element 1 (e = 1, tb <= 49: a pushed term of 2^-60 is rint(v 2^-12) = 0); maxoliters = 0 returns
    u = (M u0 + u0) / |.| after the rescale pass and the first product.  A row that is not a neighbour of the large element then
    holds 2^-60 (1 + the weights of the pairs stored in its OWN row of the copy, pulled in doubles); the pairs stored in the other
    row — about half, up_keeps' checkerboard — were pushed and are gone.  The oracle and the plain kernel keep them all.  So on the
    half copy those rows are below the oracle's, most of them by far more than a percent — an error of 1e-18, within the (c) bound
    L 2^(e - tb - 1) and within 1e-9 —, and on the plain kernel (same team) every element agrees to n 2^-47 relative."""
    reg, D1, D2, A = scored.probs[L]
    P = type(reg._abi_params()).from_buffer_copy(reg._abi_params()); P.maxoliters = 0
    u0 = np.full(L, 2.0 ** -60); u0[L // 2] = 1.0
    o = orc.register(P, D1, D2, A=A, u0=u0, faithful=False)
    ref = o["u"]
    far = (ref > 0.0) & (ref < ref.max() * 2.0 ** -40)
    assert far.sum() > L // 2 and o["stats"].nnz_upper >= HALF_COPY_MIN_PAIRS
    out = {}
    for upper in ("0", "1"):
        _one_team(monkeypatch, upper)
        _, u, _, st = _scored_solve(ctx, big, scored, L, u0, P)
        assert st.n_pass == 2 and np.all(np.isfinite(u)) and np.max(np.abs(u - ref)) <= U_TOL
        out[upper] = u
        print(f"L={L} upper={upper}: far rows {int(far.sum())}, u / u_oracle on them: median {np.median(u[far] / ref[far]):.4f}, "
              f"max {np.max(u[far] / ref[far]):.6f}, below 0.99: {int((u[far] < 0.99 * ref[far]).sum())}")
    assert np.max(np.abs(out["0"] - ref) / np.where(ref > 0, ref, 1.0)) <= L * 2.0 ** -47
    assert np.all(out["1"][far] <= ref[far] * (1 + L * 2.0 ** -47))
    assert (out["1"][far] < 0.99 * ref[far]).sum() > far.sum() // 2


@pytest.mark.parametrize("kind", ws.SCORED_STARTS)
@pytest.mark.parametrize("L", [ws.N_EDGE_LO, ws.N_EDGE_HI])
@pytest.mark.parametrize("upper", ["1", "0"], ids=["half_copy", "plain_kernel"])
def test_scored_problem_at_the_scale_edge(ctx, orc, big, scored, upper, L, kind, monkeypatch):
    """ctx.score + ctx.solve on a 'gravity' problem of L = 8192 | 8193 live associations (~0.8 M stored pairs, 16-bit labels) on one
    team of an XCD's compute units, ROMAN_WIDE_UPPER = "1": k_solve_wide<uint16_t, true> WITH the copy built (the note above; the
    test above observes it), every pass until the first column compaction over the half copy, the scale taken from the multiplied
    vector's largest element — the caller's RAW start in the first pass (twelve decades; the largest element in the last row of the
    last column block, or in the first; xmax = 2^-600 and 2^600, which give score 0 and an empty selection on both sides, see the
    dense case); = "0": k_solve_wide<uint16_t, false> on the same team.  The oracle's passes: 97 (all ones, twelve decades), 47-63
    (largest element placed), 3 (2^-600, 2^600); 0.1-0.5 s each.  The one-dominant start is not run here: on these problems the
    oracle's own u moves by 3e-11 when one element of that start moves by one ulp (tests/_wide_sums.py, SCORED_STARTS); every start
    kept is held by the oracle itself to 1e-12 or better."""
    _one_team(monkeypatch, upper)
    got = _scored_solve(ctx, big, scored, L, ws.start(kind, L))
    o = scored.ref(L, kind)
    _compare_scored(L, got, o, f"scored L={L} {kind} upper={upper}")
    if kind == "xmax_2^-600" and np.all(o["u"] > 0.0):
        assert np.max(np.abs(got[1] - o["u"]) / o["u"]) <= L * 2.0 ** -47


@pytest.mark.parametrize("upper", ["1", "0"], ids=["half_copy", "plain_kernel"])
def test_scored_problem_with_and_without_column_compaction(ctx, orc, big, scored, upper, monkeypatch):
    """Case 4 on the scored problem of L = 8193 (one team), twelve-decade start: ROMAN_WIDE_COMPACT = "0" (the half copy serves
    every pass) against "0x01FF10" (a compaction after almost every pass: the half copy serves the first only).  The pushed sums are
    integers, the pulled side and the plain kernel add doubles in pieces cut from the stream in use, so a compaction regroups
    partial sums (k_solve_wide's comment on the compaction): neither bitwise equality nor 1e-12 after ~100 passes follows from the
    code.  Each run is held to the oracle at 1e-9; the two runs select the same set after the same number of homotopy steps; their
    distance is printed."""
    L = ws.N_EDGE_HI
    _one_team(monkeypatch, upper)
    o = scored.ref(L, "decades")
    runs = []
    for compact in ("0", "0x01FF10"):
        monkeypatch.setenv("ROMAN_WIDE_COMPACT", compact)
        got = _scored_solve(ctx, big, scored, L, ws.start("decades", L))
        _compare_scored(L, got, o, f"scored L={L} upper={upper} compaction {compact}")
        runs.append(got)
    (a0, u0, _, st0), (a1, u1, _, st1) = runs
    print(f"upper={upper}: max |u(no compaction) - u(compaction every pass)| {np.max(np.abs(u0 - u1)):.3e}")
    assert sorted(map(tuple, a0.tolist())) == sorted(map(tuple, a1.tolist())) and st0.outer_iters == st1.outer_iters


@pytest.mark.parametrize("upper", [None, "1", "0"], ids=["library_choice", "half_copy", "plain_kernel"])
def test_smallest_batch_the_library_gives_the_half_copy(ctx, orc, big, scored, upper, monkeypatch):
    """roman_align_batch with the two scored problems (L = 8192 and 8193) from twelve-decade starts: two fallback problems of
    >= 8 000 live associations make one team per XCD and — with no switch — the half copy (enqueue_solve: `D.idx16 && a_teams > 0
    && maxA >= 8000`; the stored pairs are above build_upper's floor for such a team, asserted); "1" / "0" force it / the plain
    kernel on the same teams.  The batch result has no u: associations (and their order), live count, stored pairs, homotopy steps
    and score are the oracle's."""
    if upper is not None:
        monkeypatch.setenv("ROMAN_WIDE_UPPER", upper)
    Ls = (ws.N_EDGE_LO, ws.N_EDGE_HI)
    reg, D1, D2, _ = scored.probs[Ls[0]]
    feats = np.concatenate([D1, D2])
    assoc = np.concatenate([scored.probs[L][3] for L in Ls])
    u0 = np.concatenate([ws.start("decades", L) for L in Ls])
    big.held = None
    res = ctx.align_batch(reg._abi_params(), feats, [0, 0], [len(D1)] * 2, [len(D1)] * 2, [len(D2)] * 2,
                          assoc=assoc, assoc_off=[0, Ls[0], Ls[0] + Ls[1]], u0=u0)
    for b, L in enumerate(Ls):
        o = scored.ref(L, "decades"); rs = o["stats"]
        print(f"batch L={L} upper={upper}: score {res.stats['score'][b]!r} / oracle {rs.score!r}, passes {res.stats['n_pass'][b]} / {rs.n_pass}")
        assert res.status[b] == _abi.ROMAN_ST_OK and np.array_equal(res.assoc[b], o["assoc"])
        assert res.stats["n_live"][b] == L and res.stats["nnz_upper"][b] == rs.nnz_upper >= HALF_COPY_MIN_PAIRS
        assert res.stats["outer_iters"][b] == rs.outer_iters and abs(res.stats["score"][b] - rs.score) < 1e-6
