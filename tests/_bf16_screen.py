"""An independent model of the cosine stage's bf16 screen (k_cos_sel / k_cos_live, pass 1) in plain numpy: no HIP, no oracle.

  to_bf16        f64 -> f32 (round to nearest even) -> bf16 (round to nearest even on the bit pattern), as f32.  TWO steps: an offset from
                 a bf16 midpoint that is smaller than an f32 ulp is rounded away by the first, and the second then sees an exact tie.
  screen         what the kernel's pass 1 computes, with every sum in f64: the cosine of the ROUNDED rows with the rounded rows' OWN norms.
  exact_cos      the exact cosine of the rows as given: integer arithmetic on the doubles' significands, one correctly rounded division,
                 one correctly rounded square root.  exact_gate decides cos > cosine_min without any rounding at all.
  adversarial_pair / adversarial_pair_up
                 two rows whose rounding turns each row AWAY from (towards) the other: the screen under- (over-) estimates by a large part
                 of its bound 2^-7, where random rows stay within ~2^-8 / sqrt(d) of the exact cosine.

The family: |a_k| and |b_k| lie beside bf16 midpoints with significands in [1, 1.06) (the largest half-ulp relative to the value), in
the same octave for both rows; b_k has a_k's sign for a share (1 + c) / 2 of the weight, so that cos(a, b) ~ c and the component of b
perpendicular to a is (1 - c) a_k or -(1 + c) a_k — never small.  Every element is rounded against the sign of the other row's
perpendicular component: the products sum to 2^-8 (1 - c^2) per row, 2^-7 (1 - c^2) for the pair (0.75 x 2^-7 at c = 0.5; the reach
of any input is sin(theta) 2^-7).  One coordinate is free (a: a power of two, b: whatever steers the exact cosine into the interval asked for)."""
import math

import numpy as np

U_BF16 = 2.0 ** -8                 # unit roundoff of bf16 under round-to-nearest
BOUND = 2.0 ** -7                  # |screen - cos| of the rounding alone (two rows, asin(2^-8) each)
DELTA = 2.0 ** -6                  # the kernel's margin


def accumulation_term(d):
    """The kernel comment's term for the f32 accumulation of the product and of the two norms, any order."""
    return 3.0 * d * 2.0 ** -24


def to_bf16(x, mode="rne"):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        f = x.astype(np.float32)
    u = np.atleast_1d(f).view(np.uint32).astype(np.uint64)
    if mode == "rne":
        r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    elif mode == "trunc":
        r = u & np.uint64(0xFFFF0000)
    else:
        raise ValueError(mode)
    r = np.where(np.isnan(np.atleast_1d(f)), np.uint64(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(f.shape)


def screen_norms(A, mode="rne"):
    """Norms of the rounded rows (f64)."""
    Ah = to_bf16(A, mode).astype(np.float64)
    return np.sqrt(np.einsum("...k,...k->...", Ah, Ah))


def screen_matrix(A, B, mode="rne"):
    """screen() of every pair of rows; NaN where a rounded row has no norm to divide by."""
    Ah, Bh = to_bf16(A, mode).astype(np.float64), to_bf16(B, mode).astype(np.float64)
    na, nb = np.sqrt((Ah * Ah).sum(axis=1)), np.sqrt((Bh * Bh).sum(axis=1))
    with np.errstate(all="ignore"):
        return (Ah @ Bh.T) / (na[:, None] * nb[None, :])


def screen(a, b, mode="rne"):
    return float(screen_matrix(np.asarray(a, dtype=np.float64)[None, :], np.asarray(b, dtype=np.float64)[None, :], mode)[0, 0])


def _ints(x):
    """Finite doubles as integers m_k 2^e with one common e."""
    ms, es = [], []
    for v in np.asarray(x, dtype=np.float64).ravel().tolist():
        if v != v or v in (math.inf, -math.inf):
            raise ValueError("exact arithmetic needs finite elements")
        m, e = math.frexp(v)
        ms.append(int(m * 9007199254740992.0)); es.append(e - 53)      # m 2^53 is an integer
    e0 = min(es) if es else 0
    return [m << (e - e0) for m, e in zip(ms, es)], e0


def _exact_sums(a, b):
    ia, _ = _ints(a); ib, _ = _ints(b)
    if len(ia) != len(ib):
        raise ValueError("lengths differ")
    return sum(x * y for x, y in zip(ia, ib)), sum(x * x for x in ia), sum(y * y for y in ib)   # the common scales cancel in the cosine


def exact_cos(a, b):
    """cos(a, b) = a.b / (|a| |b|) from exact sums: sqrt of the correctly rounded quotient (a.b)^2 / (a.a b.b), signed.  0 for a zero row."""
    dot, aa, bb = _exact_sums(a, b)
    if aa == 0 or bb == 0 or dot == 0:
        return 0.0
    return math.copysign(math.sqrt((dot * dot) / (aa * bb)), dot)       # int / int: correctly rounded


def exact_gate(a, b, cosine_min):
    """cos(a, b) > cosine_min, decided in integers (cosine_min as the double it is)."""
    dot, aa, bb = _exact_sums(a, b)
    if aa == 0 or bb == 0:
        return 0.0 > cosine_min
    num, den = float(cosine_min).as_integer_ratio()
    if num < 0:                                                         # cos > -|c|  <=>  not (cos <= -|c|)
        return dot >= 0 or dot * dot * den * den < num * num * aa * bb
    return dot > 0 and dot * dot * den * den > num * num * aa * bb


def cos_matrix(A, B):
    """Every pair's cosine in numpy.longdouble (64-bit significand where the platform has one): within 2^-45 of the exact value for rows
    of up to 768 elements — for whole matrices; the planted pairs get exact_cos()."""
    A, B = np.asarray(A, dtype=np.longdouble), np.asarray(B, dtype=np.longdouble)
    na, nb = np.sqrt((A * A).sum(axis=1)), np.sqrt((B * B).sum(axis=1))
    with np.errstate(all="ignore"):
        return (A @ B.T) / (na[:, None] * nb[None, :])


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _balanced_signs(w, goal):
    """Signs s_k with sum s_k w_k ~ goal: the heaviest first, each towards the goal."""
    s = np.ones(len(w))
    run = 0.0
    for k in np.argsort(-w, kind="stable"):
        s[k] = 1.0 if abs(run + w[k] - goal) <= abs(run - w[k] - goal) else -1.0
        run += s[k] * w[k]
    return s


def _place(sign, expo, idx, grow, sub, contrary, rng):
    """sign 2^expo (1 + (2 idx + 1) 2^-8 +- offset): beside the midpoint of the bf16 neighbours 1 + idx 2^-7 and 1 + (idx + 1) 2^-7 on the
    side that rounds the magnitude up (grow) or down.  sub: the offset is below an f32 ulp (2^-30 ... 2^-44 of the value), f64 -> f32
    lands ON the midpoint and the tie goes to the even neighbour — idx is given the parity that sends the tie the wanted way, or, for
    `contrary` elements, the other way (the offset says up, the two-step conversion goes down: what a one-step model gets wrong)."""
    idx = idx.copy()
    tie_grows = (idx % 2) == 1                                           # the upper neighbour 1 + (idx + 1) 2^-7 is the even one
    flip = sub & (tie_grows != (grow ^ contrary))
    idx[flip] ^= 1
    off = np.where(sub, 2.0 ** -rng.integers(30, 45, size=len(idx)), 2.0 ** -rng.integers(12, 20, size=len(idx)))
    mag = 1.0 + (2.0 * idx + 1.0) * 2.0 ** -8 + np.where(grow, off, -off)
    return sign * np.ldexp(mag, expo)


def _pow2(x):
    return int(round(math.log2(x)))


def _steer(a, b, f, target):
    """b[f] := t with cos(a, b) = target in f64 (the root of smaller magnitude on the right branch); a[f] stays."""
    m = np.ones(len(a), dtype=bool); m[f] = False
    A = float(a @ a); D0 = float(a[m] @ b[m]); B0 = float(b[m] @ b[m]); af = float(a[f])
    qa, qb, qc = af * af - target * target * A, 2.0 * D0 * af, D0 * D0 - target * target * A * B0
    if target == 0.0:
        return -D0 / af
    disc = max(qb * qb - 4.0 * qa * qc, 0.0)
    roots = [(-qb + s * math.sqrt(disc)) / (2.0 * qa) for s in (1.0, -1.0)] if qa != 0.0 else [-qc / qb]
    ok = [t for t in roots if (D0 + af * t > 0) == (target > 0)]
    return min(ok or roots, key=abs)


def _tune_norm(a, top):
    """a, scaled by a power of two and extended by four elements that are bf16 values themselves, such that the ROUNDED row's sum of
    squares lies in (top (1 - 2^-26), top]: each element is the largest bf16 value whose square still fits (it leaves at most 2^-7 of the gap)."""
    ah = to_bf16(a).astype(np.float64)
    k = math.floor(0.5 * math.log2(top / float(ah @ ah)))
    while float(np.ldexp(ah, k) @ np.ldexp(ah, k)) > top:
        k -= 1
    a = np.ldexp(a, k)
    s = float(np.ldexp(ah, k) @ np.ldexp(ah, k))
    extra = []
    for _ in range(4):
        x = float(to_bf16(math.sqrt(max(top - s, 0.0)), "trunc"))
        while s + x * x > top:
            x = float(to_bf16(x * (1.0 - 2.0 ** -8), "trunc"))
        extra.append(x); s += x * x
    assert top * (1.0 - 2.0 ** -26) < s <= top
    return np.concatenate([a, extra])


def _build(rng, d, c, scale_a, scale_b, up, lo, hi, sub_share, contrary_share, octaves, norm2_a=None):
    expo = rng.integers(0, octaves, size=d)
    ia, ib = rng.integers(0, 8, size=d), rng.integers(0, 8, size=d)
    sa = rng.choice([-1.0, 1.0], size=d)
    ma, mb = np.ldexp(1.0 + (2.0 * ia + 1.0) * 2.0 ** -8, expo), np.ldexp(1.0 + (2.0 * ib + 1.0) * 2.0 ** -8, expo)
    f = int(rng.integers(0, d)) if d >= 3 else -1                        # the free coordinate
    w = ma * mb
    if f >= 0:                                                           # (a's free element: a power of two of the largest octave — it
        w[f] = 0.0; ma[f] = 2.0 ** int(expo.max()); mb[f] = 0.0          # moves the cosine by up to ~a_f^2 / (2 c |a|^2))
    rel = _balanced_signs(w, c * math.sqrt(float(ma @ ma) * float(mb @ mb)))
    a0, b0 = sa * ma, sa * rel * mb
    # the perpendicular component of the other row decides which way an element is rounded: away (up: towards)
    pb = b0 - (a0 @ b0) / (a0 @ a0) * a0
    pa = a0 - (a0 @ b0) / (b0 @ b0) * b0
    turn = -1.0 if not up else 1.0
    grow_a = np.sign(pb) * turn == np.sign(a0)                           # the rounding error of a_k has the sign turn * sign(pb_k)
    grow_b = np.sign(pa) * turn == np.sign(b0)
    sub_a, sub_b = rng.random(d) < sub_share, rng.random(d) < sub_share
    con_a, con_b = sub_a & (rng.random(d) < contrary_share), sub_b & (rng.random(d) < contrary_share)
    a = _place(np.sign(a0), expo, ia, grow_a, sub_a, con_a, rng)
    b = _place(np.sign(b0), expo, ib, grow_b, sub_b, con_b, rng)
    if f >= 0:
        a[f] = a0[f]
    if norm2_a is not None:                                              # (d + 4 elements; b has zeros where a has its four extra ones)
        a = _tune_norm(a, norm2_a); b = np.concatenate([b, np.zeros(4)])
    if f >= 0:
        b[f] = _steer(a, b, f, 0.5 * (lo + hi))
    na = math.sqrt(float(a @ a)); nb = math.sqrt(float(b @ b))
    if norm2_a is None:
        a = np.ldexp(a, _pow2(scale_a / na))                             # powers of two: the rounding pattern and the cosine stay
    return a, np.ldexp(b, _pow2(scale_b / nb))


def adversarial_pair(rng, d, c, scale_a=1.0, scale_b=1.0, lo=None, hi=None, up=False, sub_share=0.25, contrary_share=0.125, octaves=4, draws=6, norm2_a=None):
    """Rows a, b (f64, d elements, norms within a factor sqrt(2) of scale_a, scale_b) whose exact cosine lies in (lo, hi] — by default
    (c, c + 2^-10] — and whose bf16 rounding turns each row away from the other: of `draws` such pairs the one whose screen (this model's)
    lies farthest below the exact cosine.  norm2_a: a comes with d + 4 elements and the sum of the squares of its ROUNDED elements
    within 2^-26 below norm2_a (the screen's own norm, which the kernel's case split reads), b with four zeros there.  For d < 3 there is no free coordinate: the rows come as they are (cosine +-1 at d = 1)."""
    lo = c if lo is None else lo
    hi = lo + 2.0 ** -10 if hi is None else hi
    best, reach = None, -math.inf
    for _ in range(50):
        a, b = _build(rng, d, c, scale_a, scale_b, up, lo, hi, sub_share, contrary_share, octaves, norm2_a)
        e = exact_cos(a, b)
        if d >= 3 and not lo < e <= hi:
            continue
        r = (screen(a, b) - e) * (1.0 if up else -1.0)
        if r > reach:
            best, reach = (a, b), r
        draws -= 1
        if draws <= 0:
            break
    if best is None:
        raise RuntimeError(f"no pair with a cosine in ({lo}, {hi}] at d = {d}")
    return best


def adversarial_pair_up(rng, d, c, scale_a=1.0, scale_b=1.0, lo=None, hi=None, **kw):
    """The same with every element rounded TOWARDS the other row: the screen over-estimates.  Default interval: (c - 2^-10, c)."""
    hi = c if hi is None else hi
    lo = hi - 2.0 ** -10 if lo is None else lo
    return adversarial_pair(rng, d, c, scale_a, scale_b, lo=lo, hi=math.nextafter(hi, -math.inf), up=True, **kw)


def truncation_pair(rng, d, c, lo=None, hi=None):
    """The family for a TRUNCATING f32 -> bf16: truncation only shrinks, by up to a whole ulp 2^-7 — an element that should shrink sits just
    below a bf16 value (it loses the whole ulp), one that should grow sits ON one (it loses nothing)."""
    lo = c if lo is None else lo
    hi = lo + 2.0 ** -10 if hi is None else hi
    for _ in range(50):
        expo = rng.integers(0, 4, size=d)
        sa = rng.choice([-1.0, 1.0], size=d)
        f = int(rng.integers(0, d))
        w = np.ldexp(1.0, 2 * expo); w[f] = 0.0
        rel = _balanced_signs(w, c * float(w.sum()))
        a0, b0 = sa * np.ldexp(1.0, expo), sa * rel * np.ldexp(1.0, expo)
        a0[f] = 8.0; b0[f] = 0.0
        pb = b0 - (a0 @ b0) / (a0 @ a0) * a0
        pa = a0 - (a0 @ b0) / (b0 @ b0) * b0
        shrink_a, shrink_b = np.sign(pb) == np.sign(a0), np.sign(pa) == np.sign(b0)
        a = a0 * np.where(shrink_a, 1.0 + 2.0 ** -7 - 2.0 ** -16, 1.0)
        b = b0 * np.where(shrink_b, 1.0 + 2.0 ** -7 - 2.0 ** -16, 1.0)
        a[f] = 8.0
        b[f] = _steer(a, np.where(np.arange(d) == f, 0.0, b), f, 0.5 * (lo + hi))
        if lo < exact_cos(a, b) <= hi:
            return a, b
    raise RuntimeError("no truncation pair")
