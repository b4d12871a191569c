"""Case builders for tests/test_gpu_wide_sums.py and the integer model of tests/test_wide_sums_cpu.py: the sums of the
whole-device solver (k_solve_wide) at their worst case and at the size edge of the half copy's fixed-point scale.

The scale rule of the half copy (kernels.hip.h, k_solve_wide's `stream`, the block that sets fxScale, and piece_up), restated:
a pass multiplies a vector x >= 0 with largest element xmax; frexp(xmax) = (m, e), 0.5 <= m < 1, so x_p < 2^e for every p (e = 0
when xmax is 0 or not below 1e300); tb = min(49, 62 - bits(L - 1)), bits(k) the bit length of k; a stored pair (p, q, v),
0 <= v <= 1, adds the integer rint(v * x_p * 2^(tb - e)) (one rounding, ties to even) to the M accumulator of column q and
rint(x_p * 2^(tb - e)) to its C accumulator — unsigned 64-bit words in LDS; a column's sum times 2^(e - tb) is its share of the
product."""
import math

import numpy as np

STREAM_MAXL = 3072                      # the stream solver takes live sets up to here; 3073 is the first the wide solver gets
N_EDGE_LO, N_EDGE_HI = 8192, 8193       # tb = 49 | 48
DENSE_SIZES = (STREAM_MAXL + 1, N_EDGE_LO, N_EDGE_HI)
CPU_SIZES = (3073, 4096, 4097, 8192, 8193, 32767, 40000)

WORST_STARTS = ("ones", "decades", "one_dominant")                  # the stream test's three (tests/test_gpu_batch.py)
PLACED_STARTS = ("max_last", "max_first", "xmax_2^-600", "xmax_2^600")
ALL_STARTS = WORST_STARTS + PLACED_STARTS

# Passes of the oracle (pass mode `auto`: carried above STREAM_MAXL), measured on the CPU before the case list was fixed.  The
# cap for a dense problem (33 M pairs a pass) is 60.
ORACLE_PASSES = {
    # dense, M and C all ones, n = 3073 | 8192 | 8193, every start (ALL_STARTS at 8193): the rescale pass makes u uniform whatever
    # the start (M u0 + u0 = sum(u0) in every row), the first trial confirms it
    "all ones": 3,
    # dense, n = 8193, M = 2^-20, C all ones: from all ones 3 (every u equal: omega = 1 is a tie), from the twelve-decade and the
    # one-dominant start 202 (the cap of 200 inner iterations; 25 s) -> the twelve-decade start with maxiniters = 10
    "M = 2^-20, twelve decades, maxiniters 10": 12,
    # dense, n = 8192 | 8193, M uniform in (0, 1], twelve-decade start
    "random weights": 6,
    # dense, n = 8193, M all ones, C = 0 on rows [0, 64) x columns [n - 64, n): 1172 (all ones) / 1146 (twelve decades) / 1370
    # (one dominant) passes, 140-160 s with rescale_u0: the rescale pass of an all-ones M wipes out ANY start, the two sides of
    # the block are then interchangeable (every placement of the block is a relabelling of this problem) and the iteration sits on
    # the symmetric saddle for a thousand passes before rounding lets one side win.  With rescale_u0 = 0 and the start
    # `block_tilted` (every element distinct, the block's row side a quarter of the rest) the row side loses at once: 7 passes,
    # 8129 selected, the gap in u at the cut 1.1e-2, the oracle's answer unmoved (0.0) by one ulp in the start.  Capping the
    # iteration instead (rescale_u0 = 1, maxiniters 10, maxoliters 2) stops on the saddle: 37 passes, the cut inside tied elements.
    "planted block, rescale_u0 = 0, block_tilted": 7,
    # scored 'gravity' problems (0.8 M pairs: 0.1-0.5 s whatever the count), L = 8192 | 8193
    "scored: all ones, twelve decades": 97, "scored: one dominant": 141, "scored: max_last": (63, 56), "scored: max_first": (47, 50),
    "scored: xmax 2^-600, 2^600": 3,
}
# The oracle against ITSELF on the scored problems, one element of the start moved by one ulp (elements 0, 7, 1234, L - 1, up and
# down; max |du|): all ones 8e-15, twelve decades 6e-15, max_last 4e-13, max_first 8e-13 — and one dominant 2.4e-11 | 3.4e-11
# (L = 8192 | 8193): a change of 2e-28 in the input moves u by 3e-11 and the stop of the 141-pass inner loop (|dF| < tol_F) with it.
# A start whose answer the reference itself holds to no better than a thirtieth of the 1e-9 bound under one ulp is no case for that
# bound (sums in another order move every element of every product by an ulp): the scored cases take every start but that one;
# max_first / max_last (1e-9 everywhere, one element 1) are its well-conditioned neighbours.  The dense cases keep it.
# For the record, the device from that start on one team (L = 8192 | 8193; max |u - u_oracle|, passes against the oracle's 141):
# half copy 7.9e-10 | 1.2e-9 (141 | 141), plain kernel 1.6e-6 | 1.9e-11 (142 | 141) — scatter, as the oracle's own figure says.
SCORED_STARTS = tuple(k for k in ALL_STARTS if k != "one_dominant")


def start(kind, n):
    """The start vector of `kind` for a problem of n associations (None: the library's all ones)."""
    rng = np.random.default_rng(5)
    if kind == "ones":
        return None
    if kind == "decades":               # twelve decades, one element exactly 1, one exactly 1e-12
        u0 = 10.0 ** rng.uniform(-12, 0, n); u0[7] = 1.0; u0[11] = 1e-12
        return u0
    if kind == "one_dominant":
        u0 = np.full(n, 1e-12); u0[1234] = 1.0
        return u0
    if kind == "max_last":              # the largest element in the last row of the last slice and column block
        u0 = np.full(n, 1e-9); u0[n - 1] = 1.0
        return u0
    if kind == "max_first":
        u0 = np.full(n, 1e-9); u0[0] = 1.0
        return u0
    if kind == "block_tilted":          # for the planted block: every element distinct, the block's row side a quarter of the rest
        u0 = rng.uniform(0.5, 1.0, n); u0[:64] *= 0.25
        return u0
    if kind == "xmax_2^-600":          # the twelve-decade start scaled by a power of two (exact): xmax = 2^-600 / 2^600
        return np.ldexp(start("decades", n), -600)
    if kind == "xmax_2^600":
        return np.ldexp(start("decades", n), 600)
    raise ValueError(kind)


def plant_block(Cm, n):
    """C = 0 on the 64 x 64 block rows [0, 64) x columns [n - 64, n) (and its mirror) of an all-ones C, in place: the first slice
    against the last 64 associations — the odd row n - 1 of the last slice and column block among them."""
    Cm[0:64, n - 64:n] = 0.0
    Cm[n - 64:n, 0:64] = 0.0


def random_weights(M, n, seed=8):
    """Uniform weights in (0, 1], symmetric, unit diagonal, written into the leading n x n corner of M in place."""
    rng = np.random.default_rng(seed)
    V = M[:n, :n]
    for r0 in range(0, n, 1024):        # (row bands: no second n x n array, no index arrays)
        r1 = min(n, r0 + 1024)
        V[r0:r1, r0:] = 1.0 - rng.random((r1 - r0, n - r0))
        V[r0:r1, :r0] = V[:r0, r0:r1].T
        d = V[r0:r1, r0:r1]
        d[:] = np.triu(d, 1) + np.triu(d, 1).T
    np.fill_diagonal(V, 1.0)
    return V


def gravity_problem(L, seed=1230):
    """A scored problem of exactly L live associations for the half copy (which the dense entry cannot reach: 32-bit labels):
    a synthetic 'gravity' pair of 91 x 91 objects (every association live) with the explicit list of the first L associations
    of the all-to-all order.  -> (registration, D1, D2, A)."""
    from conftest import registration_for
    from roman_amd import synth
    from roman_amd.clipperpy.utils import create_all_to_all
    reg = registration_for("gravity")
    pr = synth.make_pair(91, 91, 0, seed, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    A = np.ascontiguousarray(create_all_to_all(91, 91)[:L], dtype=np.int32)
    return reg, D1, D2, A


# ---- the integer model (tests/test_wide_sums_cpu.py): Python ints only ----------------------------------------------------------

def scale_bits(L):
    """tb of a live set of L associations."""
    return min(49, 62 - max(L - 1, 1).bit_length())


def scale_exponent(xmax):
    """e of a vector whose largest element is xmax (the device's guard: 0 unless 0 < xmax < 1e300)."""
    return math.frexp(xmax)[1] if 0.0 < xmax < 1.0e300 else 0


def int_parts(a):
    """The doubles of `a` as exact (integer mantissa, exponent) pairs: a_p = m_p 2^(x_p)."""
    m, x = np.frexp(np.asarray(a, dtype=np.float64))
    mi = np.ldexp(m, 53).astype(np.int64)
    return [(int(a_), int(b_) - 53) for a_, b_ in zip(mi, x)]


def shift_rint(P, s):
    """rint(P 2^s) for an integer P >= 0: one rounding, ties to even (the device's fma(v, x 2^(tb - e), magic))."""
    if s >= 0:
        return P << s
    r = -s
    q, rem, half = P >> r, P & ((1 << r) - 1), 1 << (r - 1)
    return q + 1 if (rem > half or (rem == half and (q & 1))) else q


def pushed_sums(v, x, L):
    """What the rows p = 0 .. len(x) - 1 push for the weights v_p and the vector x of a live set of L associations.
    -> dict: terms (ints), tb, e, and the exact products v_p x_p as integers `exact` in units of 2^unit."""
    x = np.asarray(x, dtype=np.float64)
    e, tb = scale_exponent(float(x.max())), scale_bits(L)
    xs = int_parts(x)
    vs = int_parts(np.broadcast_to(np.asarray(v, dtype=np.float64), x.shape))
    prods = [(mv * mx, ev + ex) for (mv, ev), (mx, ex) in zip(vs, xs)]
    unit = min(ex for _, ex in prods)
    return dict(terms=[shift_rint(P, ex + tb - e) for P, ex in prods], tb=tb, e=e,
                exact=[P << (ex - unit) for P, ex in prods], unit=unit)


def sum_error_within_bound(S, exact_sum, unit, tb, e, L):
    """(c): |S 2^(e - tb) - exact_sum 2^unit| <= L 2^(e - tb - 1), in integers at the smaller of the two units."""
    c = min(unit, e - tb - 1)
    return abs((S << (e - tb - c)) - (exact_sum << (unit - c))) <= (L << (e - tb - 1 - c))


