"""The headroom of the half copy's fixed-point sums (k_solve_wide, pull + push passes), checked in exact integer arithmetic.

The rule is restated in tests/_wide_sums.py from the documented formula (no kernel text is read): with
frexp(xmax) = (m, e) and tb = min(49, 62 - bits(L - 1)) a stored pair (p, q, v) adds rint(v x_p 2^(tb - e)) to column q's
accumulator.  Which rows push into a column depends on the layout; the model lets EVERY other row do so (L - 1 terms: the most a
column can get), so what holds here holds for any layout.  For every size and start vector of the GPU cases:
(a) every term is below 2^49, (b) every column's sum is below 2^62, (c) the sum times 2^(e - tb) is within L 2^(e - tb - 1) of the
exact rational sum — for the weights 1 (the C accumulator, and M all ones), 2^-20 and uniform in (0, 1]."""
import numpy as np
import pytest

import _wide_sums as ws


def _weights(kind, n):
    if kind == "ones":
        return 1.0
    if kind == "2^-20":
        return 2.0 ** -20
    return 1.0 - np.random.default_rng(n).random(n)             # one column of the random-weights case: uniform in (0, 1]


def _check(v, x, L, strict_49=True):
    r = ws.pushed_sums(v, x, L)
    terms, tb, e = r["terms"], r["tb"], r["e"]
    assert tb == (49 if L <= 8192 else 62 - (L - 1).bit_length())
    assert max(terms) < (1 << 49) if strict_49 else max(terms) <= (1 << tb)                         # (a)
    T, X = sum(terms), sum(r["exact"])
    assert T - min(terms) < (1 << 62)                                                               # (b): the fullest column
    for q in {0, len(terms) - 1, int(np.argmax(x)), int(np.argmin(x))}:                             # (c): columns that miss an end or an extreme
        assert ws.sum_error_within_bound(T - terms[q], X - r["exact"][q], r["unit"], tb, e, L)
    assert ws.sum_error_within_bound(T, X, r["unit"], tb, e, L)
    return r


def test_scale_bits_at_the_edges():
    assert [ws.scale_bits(L) for L in (2, 3073, 4096, 4097, 8192, 8193, 16384, 16385, 32767, 40000, 65534)] == \
        [49, 49, 49, 49, 49, 48, 48, 47, 47, 46, 46]
    assert ws.scale_exponent(1.0) == 1 and ws.scale_exponent(0.75) == 0 and ws.scale_exponent(2.0 ** -600) == -599
    assert ws.scale_exponent(0.0) == 0 and ws.scale_exponent(1e300) == 0                            # (the device's guard)


def test_rounding_is_to_nearest_ties_to_even():
    assert [ws.shift_rint(P, -1) for P in (0, 1, 2, 3, 5, 7)] == [0, 0, 1, 2, 2, 4]
    assert ws.shift_rint(5, 3) == 40 and ws.shift_rint((1 << 60) + 1, -2) == 1 << 58


@pytest.mark.parametrize("kind", ws.ALL_STARTS)
@pytest.mark.parametrize("n", ws.CPU_SIZES)
def test_terms_and_column_sums_stay_in_range(n, kind):
    x = ws.start(kind, n)
    if x is None:
        x = np.ones(n)
    for w in ("ones", "2^-20", "random"):
        _check(_weights(w, n), x, n)


@pytest.mark.parametrize("n", ws.CPU_SIZES)
def test_the_vector_that_fills_the_headroom(n):
    """Every element just below a power of two, weight 1: frexp gives e = 0, a term rounds UP to 2^tb itself (so (a) holds as
    `<= 2^tb`, not strictly), and a column's L - 1 terms sum to (L - 1) 2^tb < 2^bits(L - 1) 2^tb <= 2^62: the bound (b) rests on
    a column never receiving its own row — L terms of 2^49 at L = 8192 would be exactly 2^62."""
    x = np.full(n, np.nextafter(1.0, 0.0))
    r = _check(1.0, x, n, strict_49=False)
    assert r["e"] == 0 and set(r["terms"]) == {1 << r["tb"]}
    if n == 8192:
        assert sum(r["terms"]) == 1 << 62
