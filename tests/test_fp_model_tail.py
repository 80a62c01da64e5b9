"""CPU checks of the FP64 mod-down tail of the fused key switch (ntt.hip ks_tail_store_fp), with the bound model of
tests/fp_model.py: on a modulus q < 2^50 the tail computes (acc - T) P^-1 + ct mod q without leaving the doubles,

    d = fp_reduce(acc) - T          |acc| <= 7.88 q (the running sums), |T| <= 5.22 q (un-reduced row stages)
    t = fp_mul(d, inv, RN(inv RN(1/q)))      inv = P^-1 mod q, canonical
    r = fp_canon(t + ct)            ct < 2^52

and the comments next to it claim |d| <= 5.72 q, |k - d inv / q| <= 2.65, |t| <= 2.65 q, every FMA and sum exact.
(The device side: tests/test_gpu_fp_tail.py.)"""
import random
from fractions import Fraction

import pytest

import fp_model as fm

B_ACC = Fraction(788, 100)   # the running sums as the digit loop leaves them
B_T = Fraction(522, 100)     # T after its un-reduced row stages
B_D = Fraction(572, 100)     # claimed: |fp_reduce(acc) - T| / q
E_T = Fraction(265, 100)     # claimed: |k - d inv / q| and |t| / q
QS = [2 ** 50 - 1, 2 ** 49 + 1, 2 ** 50 - 16383]  # the limit the plan builder admits, the bottom of the width, one in between


def test_claimed_bounds_cover_the_rigorous_ones():
    assert (B_ACC + B_T) * (2 ** 50 - 1) > 2 ** 53  # why the sums are re-centred first: acc - T can reach 13.1 q
    for q in QS:
        ks = dict(fm.sched_keyswitch(q, 16, 64, False).rows)
        # what the digit loop and the row stages hand over (the model's 7.88 carries the 2^-41 of a re-centred sum)
        assert ks["sums"] <= B_ACC + Fraction(1, 2 ** 40) and ks["s15"] <= B_T and ks["sums"] * q < 2 ** 53
        for rigorous in (False, True):
            r = fm.reduce_out(q) if rigorous else Fraction(1, 2) * (1 + Fraction(1, 2 ** 40))
            d = r + ks["s15"]
            assert d <= B_D and d * q < 2 ** 53                      # the difference of two integers below 2^53
            e = fm.quotient_error(B_D, Fraction(q - 1, q), q, "recomputed") if rigorous else Fraction(1, 2) + Fraction(3, 8) * B_D
            assert e <= E_T, (q, rigorous, float(e))
            assert fm.mul_is_exact(B_D, Fraction(q - 1, q), q, E_T)  # k < 2^53, |h - k q| < 2^53: both FMAs and the sum exact
            assert E_T * q + 2 ** 52 < 2 ** 53                       # t + ct, ct < 2^52: what fp_canon is given


@pytest.mark.parametrize("p", [11, 12])
def test_exhaustive_in_reduced_formats(p):
    """every (d, inv) pair of a format with p significand bits: 2^53 -> 2^p, 2^50 -> 2^(p-3)"""
    primes = [v for v in range(2 ** (p - 3) - 1, 2, -2) if all(v % k for k in range(3, int(v ** 0.5) + 1, 2))]
    for q in primes[:2]:
        r = fm.exhaustive_fp_mul(p, q, float(B_D), "recomputed")
        assert r["pairs"] > 0 and r["inexact"] == 0
        assert r["worst_t"] <= float(E_T) and r["worst_slope"] <= 0.375


def test_adversarial_search_in_double_precision():
    rng = random.Random(2027)
    for q in QS:
        worst, exact = fm.search_fp_mul(q, B_D, "recomputed", rng, 6000)
        assert exact and worst <= fm.quotient_error(B_D, Fraction(q - 1, q), q, "recomputed") <= E_T, (q, float(worst))
        assert worst > Fraction(3, 4)  # the search is not vacuous: well beyond the 1/2 of an exact quotient


def _tail(acc, tv, inv, ct, q):
    """ks_tail_store_fp on one coefficient, every step checked for exactness"""
    qi = 1.0 / float(q)
    r, ok = fm.fp_reduce(float(acc), q, qi)
    assert ok and 2 * abs(r) <= q * (1 + 2.0 ** -40)
    d = r - float(tv)
    assert int(d) == int(r) - tv and abs(d) <= float(B_D) * q
    t, k, ok = fm.fp_mul(d, float(inv), fm.companion_recomputed(inv, q), q)
    assert ok and abs(t) <= float(E_T) * q
    s = t + float(ct)
    assert int(s) == int(t) + ct and abs(s) < 2 ** 53
    o, ok = fm.fp_reduce(s, q, qi)
    assert ok
    o = o + float(q) if o < 0 else o
    assert 0 <= o < q
    return int(o)


def test_the_residue_is_the_integer_form_s():
    """(acc - T) P^-1 + ct mod q in Python integers against the FP64 sequence: operands at their largest magnitudes,
    the added term 0, q - 1 and (beyond what the operators pass) anything below 2^52, inverses next to 0, q / 2 and q"""
    rng = random.Random(7)
    for q in QS:
        amax, tmax = int(B_ACC * q), int(B_T * q)
        invs = [1, 2, q // 2, q // 2 + 1, q - 2, q - 1] + [rng.randrange(1, q) for _ in range(6)]
        accs = [amax, -amax, amax - 1, q // 2, -(q // 2), 0] + [rng.randrange(-amax, amax + 1) for _ in range(40)]
        tvs = [tmax, -tmax, 1 - tmax, 0, q - 1] + [rng.randrange(-tmax, tmax + 1) for _ in range(40)]
        cts = [0, q - 1, 1, 2 ** 52 - 1, q] + [rng.randrange(0, q) for _ in range(4)]
        for inv in invs:
            for i in range(200):
                acc, tv, ct = accs[i % len(accs)], tvs[(i * 7 + i // len(accs)) % len(tvs)], cts[i % len(cts)]
                assert _tail(acc, tv, inv, ct, q) == ((acc - tv) * inv + ct) % q, (q, acc, tv, inv, ct)
