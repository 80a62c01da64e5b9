"""EvalMod of CKKS bootstrapping as a plan (heongpu_amd/csrc/poly_eval.cpp eval_mod_plan; host only, no GPU).

The input register holds u = (I + eps) / K, I an integer with |I| < K.  With c = (1 / 2 pi)^(1 / 2^r) the plan evaluates
the degree-d Chebyshev interpolant p of g(u) = c cos(2 pi (K u - 1/4) / 2^r) and then r double-angle steps
y <- 2 y^2 - c^(2^(i+1)); y_r = sin(2 pi eps) / 2 pi.  `model` below is that computation with numpy alone
(chebinterpolate, chebval, the recurrence in doubles); `run_plan` interprets the plan's steps in doubles on value * scale.

Bounds, K = 6, degree 30, r = 3, |eps| <= 2^-10, every |I| <= 5:
  * |y_r - sin(2 pi eps) / 2 pi| <= 1e-12.  The numpy model alone gives 6.2e-15 (printed below); the plan adds the
    rounding of its integer weights at scale 2^50, at most 31 terms of 2^-51 each through an amplification of 2^r by the
    double angles: below 1.2e-13.  Observed: 1.6e-14.
  * |y_r - eps| <= (2 pi)^2 2^-30 / 6 * 1.01 = 6.19e-9, the cubic term of the sine.
K = 12 and 16 at the same degree: the bound of the first check is the model's own error (printed) plus the 1e-12 of the
weights.  K = 16 at degree 30 is under-resolved (the model itself is off by about 1e-9), which the test records.

As in test_poly_eval_plan.py the arithmetic is checked with moduli equal to the scale (2^50): a Chebyshev tail 2 T_a T_b -
T_c subtracts registers whose scale labels differ by |q / 2^50 - 1| with real primes, the approximation the evaluator
accepts and far above 1e-12.  Structure, levels, scales and tail constants are checked with real primes."""
import ctypes
import math

import numpy as np
import pytest

import heongpu_amd as hg
from heongpu_amd import _lib, api

SCALE = 2.0 ** 50
FLAT_PRIMES = [1 << 50] * 13
REAL_PRIMES = [(1 << 50) + k * 8192 + 1 for k in (3, 4, 7, 9, 12, 16, 18, 19, 21, 22, 24, 27, 31)]
DEGREE, R, LEVEL = 30, 3, 12


def g_coeffs(K, degree, r):
    c = (1.0 / (2.0 * math.pi)) ** (1.0 / 2 ** r)
    return np.polynomial.chebyshev.chebinterpolate(lambda u: c * np.cos(2 * np.pi * (K * u - 0.25) / 2 ** r), degree), c


def model(K, degree, r, u):
    coeffs, c = g_coeffs(K, degree, r)
    y = np.polynomial.chebyshev.chebval(u, coeffs)
    for i in range(r):
        y = 2 * y * y - c ** (2 ** (i + 1))
    return y


def run_plan(plan, primes, u, scale):
    regs = [u * scale]
    for s in plan.steps:
        if s.kind == api.POLY_POWER:
            v = regs[s.a] * regs[s.b] / primes[s.mul_level]
            if s.c == api.POLY_TAIL_ONE:
                v = 2 * v - round(s.tail_const)
            elif s.c >= 0:
                v = 2 * v - regs[s.c]
        elif s.kind == api.POLY_LEAF:
            v = np.full_like(u, s.w0[0])
            for i in range(s.n_terms):
                v = v + s.w[i][0] * regs[s.term_reg[i]]
        else:
            q = regs[s.a]
            if s.rescale_first:
                q = q / primes[plan.steps[s.a - 1].level]
            v = q * regs[s.b] + regs[s.c]
            if s.rescale_after:
                v = v / primes[s.level + 1]
        regs.append(v)
    return regs[-1] / plan.scale


def inputs(K, seed):
    rng = np.random.default_rng(seed)
    us, eps_all = [], []
    for I in range(-(K - 1), K):
        eps = np.concatenate([rng.uniform(-2.0 ** -10, 2.0 ** -10, 61), [-2.0 ** -10, 0.0, 2.0 ** -10]])
        us.append((I + eps) / K)
        eps_all.append(eps)
    return np.concatenate(us), np.concatenate(eps_all)


def test_k6_degree30_r3_accuracy():
    u, eps = inputs(6, 1)
    assert np.max(np.abs(u)) <= 1.0
    want = np.sin(2 * np.pi * eps) / (2 * np.pi)
    m_err = np.max(np.abs(model(6, DEGREE, R, u) - want))
    plan = hg.eval_mod_plan(6, DEGREE, R, LEVEL, SCALE, SCALE, FLAT_PRIMES)
    got = run_plan(plan, [float(p) for p in FLAT_PRIMES], u, SCALE)
    err, lin = np.max(np.abs(got - want)), np.max(np.abs(got - eps))
    print(f"K 6: model {m_err:.3e} plan {err:.3e} against eps {lin:.3e}")
    assert err <= 1e-12
    assert lin <= (2 * np.pi) ** 2 * 2.0 ** -30 / 6 * 1.01


@pytest.mark.parametrize("K", [12, 16])
def test_larger_K_is_as_good_as_the_interpolant(K):
    u, eps = inputs(K, K)
    want = np.sin(2 * np.pi * eps) / (2 * np.pi)
    m_err = np.max(np.abs(model(K, DEGREE, R, u) - want))
    plan = hg.eval_mod_plan(K, DEGREE, R, LEVEL, SCALE, SCALE, FLAT_PRIMES)
    err = np.max(np.abs(run_plan(plan, [float(p) for p in FLAT_PRIMES], u, SCALE) - want))
    print(f"K {K}: model {m_err:.3e} plan {err:.3e}")
    assert err <= m_err + 1e-12
    if K == 16:
        assert m_err > 1e-10  # degree 30 does not resolve K = 16: the interpolant, not the plan, sets the error


@pytest.mark.parametrize("r", [0, 1, 3])
def test_structure_levels_scales_and_tails(r):
    K, target = 6, 2.0 ** 48
    plan = hg.eval_mod_plan(K, DEGREE, r, LEVEL, SCALE, target, REAL_PRIMES)
    depth_p = int(DEGREE).bit_length()
    level_p = LEVEL - depth_p
    target_p = target
    for i in range(r):  # the square-root chain
        target_p = math.sqrt(target_p * float(REAL_PRIMES[level_p - r + i + 1]))
    coeffs, c = g_coeffs(K, DEGREE, r)
    p = hg.poly_eval_plan(hg.CHEBYSHEV, coeffs, LEVEL, SCALE, target_p, REAL_PRIMES)
    assert len(plan.steps) == len(p.steps) + r
    for got, want in zip(plan.steps, p.steps):  # the same schedule; the weights differ in the last bits of the coefficients
        assert (got.kind, got.dst, got.a, got.b, got.c, got.level, got.mul_level, got.rescale_first, got.rescale_after,
                got.n_terms) == (want.kind, want.dst, want.a, want.b, want.c, want.level, want.mul_level, want.rescale_first,
                                 want.rescale_after, want.n_terms)
        assert got.scale == want.scale
        for i in range(got.n_terms):  # coefficients equal to 1e-14 (two sums of 31 doubles of size one), times the weight's scale ratio
            ratio = got.scale / ([SCALE] + [st.scale for st in plan.steps])[got.term_reg[i]]
            assert got.term_reg[i] == want.term_reg[i] and got.w[i][1] == 0
            assert abs(got.w[i][0] - want.w[i][0]) <= 1e-14 * ratio + 1
    last_p = plan.steps[len(p.steps) - 1]
    assert last_p.level == level_p and last_p.scale == pytest.approx(target_p, rel=1e-12)
    prev, cc = last_p, c
    for i in range(r):
        s = plan.steps[len(p.steps) + i]
        cc = cc * cc
        assert (s.kind, s.dst, s.a, s.b, s.c) == (api.POLY_POWER, len(p.steps) + i + 1, prev.dst, prev.dst, api.POLY_TAIL_ONE)
        assert (s.mul_level, s.level, s.rescale_after, s.n_terms) == (prev.level, prev.level - 1, 0, 0)
        assert s.scale == prev.scale * prev.scale / float(REAL_PRIMES[prev.level])
        assert s.tail_const == pytest.approx(cc * s.scale, rel=1e-14)
        prev = s
    assert cc == pytest.approx(1 / (2 * math.pi), rel=1e-14) or r == 0
    assert (plan.level, plan.out_limbs) == (level_p - r, level_p - r + 1 + (1 if r == 0 else 0))
    assert plan.scale == pytest.approx(target, rel=1e-12)  # the requested scale


def c_call(K=6, degree=DEGREE, r=R, level=LEVEL, scale=SCALE, target=SCALE, primes=REAL_PRIMES, fill_steps=None):
    lib = _lib.load()
    arr = (ctypes.c_uint64 * len(primes))(*primes)
    args = (K, degree, r, level, scale, target, arr, len(primes))
    if fill_steps is None:
        count = ctypes.c_int(-7)
        return lib.hegpu_eval_mod_plan_size(*args, ctypes.byref(count)), count.value
    return lib.hegpu_eval_mod_plan_fill(*args, fill_steps, len(fill_steps)), None


REFUSALS = {
    "K below 1": dict(K=0),
    "negative double angle": dict(r=-1),
    "double angle above 8": dict(r=9),
    "degree below 2": dict(degree=1),
    "degree above 255": dict(degree=256),
    "too few levels": dict(level=7),              # 5 for the polynomial + 3 double angles
    "too few levels for the double angles": dict(level=5, r=1),
    "no such level": dict(level=13),
    "an infinite scale": dict(scale=float("inf")),
    "a scale that is not a number": dict(scale=float("nan")),
    "a scale of zero": dict(scale=0.0),
    "a target scale that is not a number": dict(target=float("nan")),
    "an infinite target scale": dict(target=float("inf")),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(why):
    kw = REFUSALS[why]
    rc, count = c_call(**kw)
    assert rc == hg.E_INVALID and count == -7
    steps = (_lib.PolyStep * 4)()
    ctypes.memset(steps, 0xA5, ctypes.sizeof(steps))
    before = bytes(steps)
    rc, _ = c_call(fill_steps=steps, **kw)
    assert rc == hg.E_INVALID and bytes(steps) == before
    a = dict(K=6, degree=DEGREE, r=R, level=LEVEL, scale=SCALE, target=SCALE)
    a.update(kw)
    with pytest.raises(hg.HEError) as e:
        hg.eval_mod_plan(a["K"], a["degree"], a["r"], a["level"], a["scale"], a["target"], REAL_PRIMES)
    assert e.value.code == hg.E_INVALID


def test_fill_wants_the_size_that_size_gives():
    rc, count = c_call()
    assert rc == 0 and count > R
    steps = (_lib.PolyStep * (count - 1))()
    ctypes.memset(steps, 0xA5, ctypes.sizeof(steps))
    before = bytes(steps)
    rc, _ = c_call(fill_steps=steps)
    assert rc == hg.E_INVALID and bytes(steps) == before
    lib = _lib.load()
    assert lib.hegpu_eval_mod_plan_size(6, DEGREE, R, LEVEL, SCALE, SCALE, None, 13, ctypes.byref(ctypes.c_int(0))) == hg.E_INVALID
