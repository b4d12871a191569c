"""The model of the bf16 cosine screen (tests/_bf16_screen.py) on the CPU — what tests/test_gpu_cos_screen_adversarial.py stands on:
  * to_bf16 is torch's f64 -> f32 -> bf16 bit for bit, at midpoints, beside them by less than an f32 ulp, at the edges of the formats;
  * the kernel comment's derivation, independently of the kernel: |screen - cos| <= 2^-7 + 3 d 2^-24 over random rows and the adversarial
    families, at every descriptor length and across the norms the screen is trusted for;
  * a CONDITION ON THE INPUTS, not a measurement: the adversarial family reaches at least half the bound (2^-8) at cosine_min = 0.5 and
    0.4 sin(theta) 2^-7 at 0.6 and 0.8 — random rows reach about a fiftieth, and a margin of 2^-8 or 2^-10 would pass every test built on them;
  * what a truncating f32 -> bf16 would do to the screen."""
import math

import numpy as np
import pytest

import _bf16_screen as m

DIMS = [1, 7, 15, 32, 70, 128, 512, 515, 768]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_to_bf16_is_torchs_two_step_conversion_bit_for_bit():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    grid = np.ldexp(1.0 + np.arange(128) * 2.0 ** -7, rng.integers(-130, 125, size=128))           # bf16 values (some subnormal in bf16)
    mid = grid * (1.0 + 2.0 ** -8 / (1.0 + np.arange(128) * 2.0 ** -7))                            # the midpoints above them
    f32_to_mid = mid * (1.0 + rng.choice([-1.0, 1.0], size=128) * 2.0 ** -26)                      # f64 -> f32 lands ON the midpoint
    xs = np.concatenate([
        rng.standard_normal(4000) * np.exp2(rng.integers(-60, 60, size=4000)),
        mid, -mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf), -np.nextafter(mid, np.inf), f32_to_mid, -f32_to_mid,
        np.ldexp(1.0 + rng.random(500), rng.integers(-149, -120, size=500)),                       # subnormal in f32 / bf16
        [2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * 1.0000001, 2.0 ** -149, 2.0 ** -150, 2.0 ** -151, 1e-320, 5e-324],
        [0.0, -0.0, np.inf, -np.inf, np.nan, 3.3895313892515355e38, 3.4e38, 3.4028234663852886e38, 3.402823466385289e38, 1e39, -1e300],
    ])
    want = torch.tensor(xs, dtype=torch.float64).float().bfloat16().float().numpy()
    got = m.to_bf16(xs)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])              # (a NaN stays a NaN; its payload is nobody's contract)
    # the trap: beside a midpoint by less than an f32 ulp the first step lands on the tie and the SECOND decides (ties to even) — a
    # one-step f64 -> bf16 rounding would follow the offset instead
    up = np.ldexp(1.0 + 3 * 2.0 ** -8 - 2.0 ** -40, 5)          # just BELOW the midpoint of 1 + 2^-7 (odd) and 1 + 2^-6 (even): goes UP
    dn = np.ldexp(1.0 + 1 * 2.0 ** -8 + 2.0 ** -40, 5)          # just ABOVE the midpoint of 1 (even) and 1 + 2^-7 (odd): goes DOWN
    assert m.to_bf16(up) == np.float32(32.0 * (1.0 + 2.0 ** -6)) and m.to_bf16(dn) == np.float32(32.0)
    assert m.to_bf16(up, "trunc") == np.float32(32.0 * (1.0 + 2.0 ** -7)) and m.to_bf16(dn, "trunc") == np.float32(32.0)


def test_exact_cos_is_exact():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    for d in (1, 3, 33, 200):
        a = rng.standard_normal(d) * np.exp2(rng.integers(-30, 30, size=d)); b = rng.standard_normal(d) * np.exp2(rng.integers(-30, 30, size=d))
        fa, fb = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
        dot, aa, bb = sum(x * y for x, y in zip(fa, fb)), sum(x * x for x in fa), sum(y * y for y in fb)
        q = dot * dot / (aa * bb)
        want = math.copysign(math.sqrt(q.numerator / q.denominator), dot)
        assert m.exact_cos(a, b) == want
        for cm in (0.5, 0.0, -0.25, want, math.nextafter(want, 2.0), math.nextafter(want, -2.0)):
            strictly = dot > 0 and q > Fraction(cm) ** 2 if cm >= 0 else dot >= 0 or q < Fraction(cm) ** 2
            assert m.exact_gate(a, b, cm) == strictly, (d, cm)
    assert m.exact_cos(np.zeros(4), np.ones(4)) == 0.0 and m.exact_cos([1.0, 0.0], [0.0, 1.0]) == 0.0
    assert m.exact_cos([3e-200, 4e-200], [3e200, 4e200]) == 1.0


def _families(rng, d, scale_a, scale_b):
    yield "random", (rng.standard_normal(d) * scale_a, rng.standard_normal(d) * scale_b)
    u = rng.standard_normal(d)
    yield "clustered", ((u + 0.6 * rng.standard_normal(d)) * scale_a, (u + 0.6 * rng.standard_normal(d)) * scale_b)
    if d >= 3:
        for c in (0.5, 0.6, 0.8, 0.0, -0.3):
            yield f"under{c}", m.adversarial_pair(rng, d, c, scale_a, scale_b, draws=2)
            yield f"over{c}", m.adversarial_pair_up(rng, d, c, scale_a, scale_b, draws=2)
    else:
        yield "under", m.adversarial_pair(rng, d, 0.5, scale_a, scale_b)


@pytest.mark.parametrize("d", DIMS)
def test_the_screen_stays_within_the_kernel_comments_bound(d):
    """|cos(a^, b^) - cos(a, b)| <= 2^-7 + 3 d 2^-24 (the second term is the kernel's f32 accumulation, which this model does not have: the
    rounding alone must stay within the first, and does with room for the second-order terms)."""
    rng = np.random.default_rng(100 + d)
    worst = 0.0
    for ea, eb in [(0, 0), (40, -40), (-40, 40), (39, 39), (-39, -39), (17, -3)]:
        for name, (a, b) in _families(rng, d, 2.0 ** ea, 2.0 ** eb):
            na, nb = m.screen_norms(a), m.screen_norms(b)
            if not (2.0 ** -40 <= na <= 2.0 ** 40 and 2.0 ** -40 <= nb <= 2.0 ** 40):
                a, b = a * 0.5 if na > 1 else a * 2.0, b * 0.5 if nb > 1 else b * 2.0       # (norms within sqrt(2) of the scale: back inside)
            err = abs(m.screen(a, b) - m.exact_cos(a, b))
            worst = max(worst, err)
            assert err <= m.BOUND + m.accumulation_term(d), (name, ea, eb, err)
    print(f"d = {d}: largest |screen - cos| = {worst:.6f} = {worst / m.BOUND:.3f} x 2^-7")


@pytest.mark.parametrize("d", [d for d in DIMS if d >= 15])
def test_the_adversarial_family_reaches_into_the_margin(d):
    """The inputs' own condition: without it the GPU tests would be as toothless as tests with random rows."""
    rng = np.random.default_rng(200 + d)
    for c, need in [(0.5, 2.0 ** -8), (0.6, 0.4 * math.sqrt(1 - 0.36) * 2.0 ** -7), (0.8, 0.4 * math.sqrt(1 - 0.64) * 2.0 ** -7)]:
        for trial in range(4):
            a, b = m.adversarial_pair(rng, d, c)
            e = m.exact_cos(a, b)
            assert c < e <= c + 2.0 ** -10
            under = e - m.screen(a, b)
            print(f"d = {d} c = {c}: under-estimate {under:.6f} = {under / m.BOUND:.3f} x 2^-7 (needs {need / m.BOUND:.3f})")
            assert under >= need, (c, trial, under / m.BOUND)
            a, b = m.adversarial_pair_up(rng, d, c)
            e = m.exact_cos(a, b)
            assert c - 2.0 ** -10 < e < c
            assert m.screen(a, b) - e >= need, (c, trial)
    # random rows: two orders of magnitude less
    a = rng.standard_normal(d); b = 0.5 * a / np.linalg.norm(a) + math.sqrt(0.75) * rng.standard_normal(d) / math.sqrt(d)
    assert abs(m.screen(a, b) - m.exact_cos(a, b)) < 2.0 ** -10


def test_the_family_holds_elements_that_only_the_two_step_conversion_rounds_right():
    """Elements beside a midpoint by less than an f32 ulp, some of them on the side that a one-step rounding would send the other way."""
    rng = np.random.default_rng(7)
    a, b = m.adversarial_pair(rng, 512, 0.5)
    two = m.to_bf16(a)
    f32 = a.astype(np.float32)
    on_tie = (_bits(f32) & 0xFFFF) == 0x8000                                  # f64 -> f32 landed on a bf16 midpoint
    one_step = np.where(np.abs(a) > np.abs(f32.astype(np.float64)), np.nextafter(f32, np.float32(np.inf) * np.sign(f32)), f32)
    one = m.to_bf16(np.where(on_tie, one_step.astype(np.float64), a))         # the offset's side decides, as one rounding would
    assert on_tie.sum() >= 64 and (one != two).sum() >= 4
    assert (~on_tie).sum() >= 256


@pytest.mark.parametrize("d", [15, 70, 512])
def test_what_a_truncating_conversion_does(d):
    """Why the kernel's comment insists on round-to-nearest-even, in figures.  Truncation doubles the unit roundoff (an element loses up to
    2^-7 of its value) — but only ever SHRINKS: r_k in [0, 2^-7] is a uniform shrink by 2^-8, which turns nothing and which the rounded
    rows' own norms divide out, plus a part in [-2^-8, 2^-8] — the same turn of at most asin(2^-8) per row as under round-to-nearest, and
    the same bound 2^-7 for the screen.  So a truncating toolchain would NOT break the margin; what it breaks is the agreement of the
    device's screen with this model, element by element: the family built for truncation reaches most of the bound under `trunc`, nothing
    under `rne`, and the device test (a) fails on either family by a factor of 50 and more if the conversion is the other one."""
    rng = np.random.default_rng(300 + d)
    for c in (0.5, 0.0):
        a, b = m.truncation_pair(rng, d, c)
        e = m.exact_cos(a, b)
        t, r = m.screen(a, b, "trunc"), m.screen(a, b, "rne")
        rel = np.max(np.abs(m.to_bf16(a, "trunc").astype(np.float64) - a) / np.abs(a))
        print(f"d = {d} c = {c}: truncation under-estimates by {(e - t) / m.BOUND:.3f} x 2^-7, rne by {(e - r) / m.BOUND:.3f} x 2^-7; element error {rel / m.U_BF16:.3f} x 2^-8")
        assert rel > 1.9 * m.U_BF16                                           # twice round-to-nearest's unit roundoff, element by element
        assert e - t >= 0.4 * math.sqrt(1 - c * c) * m.BOUND                  # the family does reach into the bound under truncation ...
        assert abs(e - t) <= m.BOUND + m.accumulation_term(d)                 # ... and stays within the SAME bound
        assert abs(t - r) > 50 * (m.accumulation_term(d) + 2.0 ** -22)       # test (a)'s tolerance tells the two conversions apart
        a, b = m.adversarial_pair(rng, d, c)                                  # and so it does on the round-to-nearest family
        assert abs(m.screen(a, b, "trunc") - m.screen(a, b, "rne")) > 50 * (m.accumulation_term(d) + 2.0 ** -22)
