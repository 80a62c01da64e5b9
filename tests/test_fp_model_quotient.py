"""CPU check of the companion-free FP64 product (fpmod.cuh fp_mul_nc) that the fused key-switch row pass uses for its
butterflies, its digit x key products and its mod-down tail (ntt.hip ks_fp_row / ks_row_mac_fp_body / ks_tail_store_fp):

    h = RN(y w), l = y w - h (FMA), k = rint(RN(h RN(1/q))), t = fma(-k, q, h) + l

in exact rational arithmetic, every FMA emulated exactly (the exact value, then ONE rounding to double).  Claimed next
to the code: t == y w - k q exactly, an integer, |t| <= (0.5 + 0.375 |y| / q) q -- for |y| up to each bound the row pass
states (0.5, 1.19, 2.13, 3.43, 5.22 q at the stages and the product, 5.72 q in the tail) and 0 <= w < q < 2^50.

The digit x key product passes the key (< q) as y and the un-reduced digit (|x| <= 5.22 q) as w; the product commutes
bit for bit (h, l, k and t are symmetric in y and w), so the cases below cover it with the roles exchanged.

Also the one-instruction conversion fp_from_u64_ldexp: the raw bits of v < 2^52 are the denormal v 2^-1074, which
ldexp by 1074 scales to v exactly."""
import random
from fractions import Fraction

import numpy as np
import pytest

import tail_inputs as ti

N = 1 << 16
BOUNDS = [Fraction(50, 100), Fraction(119, 100), Fraction(213, 100), Fraction(343, 100), Fraction(522, 100), Fraction(572, 100)]
RANDOM_W = 24  # seeded random twiddles per (modulus, |y|)


def _rn(v):
    """round-to-nearest-even of an exact rational / integer to a double (CPython: correctly rounded, ties to even)"""
    return float(v) if isinstance(v, int) else v.numerator / v.denominator


def _fma(a, b, c):
    """fma(a, b, c) on doubles: the exact a b + c, one rounding"""
    return _rn(Fraction(a) * Fraction(b) + Fraction(c))


def fp_mul_nc(y, w, q):
    """fpmod.cuh fp_mul_nc on integer-valued doubles y, w.  Returns (t, k): doubles, exactly as the device forms them."""
    qd = float(q)
    qi = 1.0 / qd                        # make_fc: RN(1 / q)
    h = y * w                            # RN(y w)
    l = _fma(y, w, -h)
    k = float(round(h * qi))             # rint: Python's round() of a float is exact and half-to-even
    t = _fma(-k, qd, h) + l
    return t, k


def _is_prime(v):
    if v < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if v % p == 0:
            return v == p
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(r - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def _primes_from(start, step, count):
    out, v = [], start
    while len(out) < count:
        if _is_prime(v):
            out.append(v)
        v += step
    return out


@pytest.fixture(scope="module")
def moduli(hg):
    """every FP64 modulus of the C4 chain ({60, 50 x 15 | 60}, N = 2^16), primes just below 2^50 and just above 2^30"""
    c = hg.Context.from_bit_sizes(hg.CKKS, N, ti.C4_CHAIN[0], ti.C4_CHAIN[1], sec=hg.SEC_NONE)
    chain = [int(v) for v in c.table("modulus")]
    fp = [q for q in chain if q < 2 ** 50]
    assert len(chain) == 17 and len(fp) == 15, chain
    below = _primes_from(2 ** 50 - 1, -2, 3)
    above = _primes_from(2 ** 30 + 1, 2, 3)
    assert all(2 ** 50 - 2 ** 12 < q < 2 ** 50 for q in below) and all(2 ** 30 < q < 2 ** 30 + 2 ** 12 for q in above)
    return fp + below + above


def _cases(q, rng):
    """(y, w): |y| at and just inside each bound, both signs; w in {0, 1, q - 1, random}"""
    ws = [0, 1, q - 1] + [rng.randrange(2, q - 1) for _ in range(RANDOM_W)]
    for b in BOUNDS:
        ymax = int(b * q)  # the largest integer with |y| <= b q
        assert Fraction(ymax, q) <= b < Fraction(ymax + 1, q) and ymax < 2 ** 53
        for y in (ymax, ymax - 1, ymax - rng.randrange(2, 1 << 20)):
            for w in ws:
                yield y, w
                yield -y, w


def test_quotient_from_the_rounded_product_is_exact_and_bounded(moduli):
    rng = random.Random(20261)
    count, k_differs = 0, 0
    for q in moduli:
        for y, w in _cases(q, rng):
            yd, wd = float(y), float(w)
            assert int(yd) == y and int(wd) == w  # the operands are doubles
            t, k = fp_mul_nc(yd, wd, q)
            ti_, ki = int(t), int(k)
            assert t == ti_ and abs(k) < 2.0 ** 53, (q, y, w)                                  # an integer
            assert ti_ == y * w - ki * q, (q, y, w, t, k)                                      # exact
            assert Fraction(abs(ti_)) <= (Fraction(1, 2) + Fraction(3, 8) * Fraction(abs(y), q)) * q, (q, y, w, t)  # bounded
            assert ti_ % q == y * w % q
            # the roles exchanged (the digit x key product): the same bits
            assert fp_mul_nc(wd, yd, q) == (t, k)
            # against the form it replaces, rint(RN(y RN(w RN(1/q)))): another k now and then, the same residue
            k_old = round(yd * (wd * (1.0 / float(q))))
            k_differs += k_old != ki
            assert (y * w - k_old * q - ti_) % q == 0
            count += 1
    assert count == len(moduli) * len(BOUNDS) * 3 * (3 + RANDOM_W) * 2  # every case counted, none skipped
    assert k_differs > 0  # the comparison is not vacuous: the two quotients do differ now and then


def test_products_at_the_bound_stay_below_2_53(moduli):
    """what the exactness rests on, in rationals: |k| < 2^53 and |h - k q| <= |t| + ulp(h) / 2 < 2^52 at the largest
    operands (|y| <= 5.72 q, w < q < 2^50)"""
    for q in moduli:
        b = BOUNDS[-1]
        e = Fraction(1, 2) + Fraction(3, 8) * b
        assert b * q + e < 2 ** 53
        assert e * q + 2 ** 49 < 2 ** 52  # ulp(h) / 2 <= 2^49 for |h| < 2^103 (5.72 < 8)


def test_ldexp_conversion_is_exact(moduli):
    """fp_from_u64_ldexp: ldexp(bits-as-double, 1074) == v for v < 2^52, through numpy.ldexp on the raw bits"""
    vals = [0, 1, 2 ** 52 - 1, 2 ** 51, 2 ** 51 + 1]
    for q in moduli:
        vals += [q - 1, q // 2]
    v = np.array(vals, dtype=np.uint64)
    assert int(v.max()) < 2 ** 52
    d = np.ldexp(v.view(np.float64), 1074)
    assert d.dtype == np.float64
    assert [int(x) for x in d] == vals
    # the same values through the OR-into-the-mantissa form (fp_from_u64)
    d2 = (v | np.uint64(0x4330000000000000)).view(np.float64) - 4503599627370496.0
    assert np.array_equal(d.view(np.uint64), d2.view(np.uint64))
