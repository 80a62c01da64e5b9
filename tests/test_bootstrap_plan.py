"""The plan of the CKKS refresh (heongpu_amd/csrc/bootstrap_plan.cpp; host only, no GPU): every level and scale label
between the exhausted ciphertext and the refreshed one.

The model below follows one coefficient a through the refresh in doubles, independently of the labels the plan reports:
the integer t = D' a + q_0 I that the raise leaves (D' = k1 D), times cts_scale[f] / q per CoeffToSlot factor, through the
EvalMod plan's steps interpreted on value * scale (`run_plan`, as tests/test_eval_mod_plan.py), times stc_scale[g] / q per
SlotToCoeff factor, and at the end divided by the CALLER's scale D -- the relabelling eval_out_scale -> stc_in_scale never
touches the number, so a label that is off anywhere shows as a wrong value.  As there, the arithmetic is checked with flat
primes (every modulus 2^50, the sine scale): with real primes the Chebyshev tails subtract registers whose labels differ
by |q / 2^50 - 1|, far above the bounds here.

Bounds (K = 12 and 16, degree 30, r = 3, ratio 256, D = 2^40: k1 = 4, rho = q_0 / D' = 256, |a| <= 0.5, every |I| < K):
  * out_scale equals D to 1e-12 relative (two cube roots and a dozen products of doubles: a few 1e-16);
  * the value equals f(a) = (rho / 2 pi) sin(2 pi a / rho) to the interpolant's own error (numpy model alone, printed)
    times rho plus 1e-12 rho (the plan's rounded weights, as test_eval_mod_plan.py);
  * |f(a) - a| <= (2 pi)^2 |a|^3 / (6 rho^2) * 1.01, the cubic term of the sine.
Real primes: levels, k1 and the per-factor scales on the two 18-limb chains of tests/test_gpu_bootstrap.py."""
import ctypes
import math

import numpy as np
import pytest

import heongpu_amd as hg
from heongpu_amd import _lib, api

N = 4096
DELTA = 2.0 ** 40
FLAT = [1 << 50] * 18
CHAIN_A = ([50, 40, 40, 40, 40, 40] + [50] * 8 + [50] + [50] * 3, [60])
CHAIN_B = ([60, 40, 40, 40, 40, 40] + [60] * 8 + [56] + [56] * 3, [60])


def model(K, degree, r, u):
    c = (1.0 / (2.0 * math.pi)) ** (1.0 / 2 ** r)
    coeffs = np.polynomial.chebyshev.chebinterpolate(lambda x: c * np.cos(2 * np.pi * (K * x - 0.25) / 2 ** r), degree)
    y = np.polynomial.chebyshev.chebval(u, coeffs)
    for i in range(r):
        y = 2 * y * y - c ** (2 ** (i + 1))
    return y


def run_steps(steps, primes, x):
    """the plan's steps on value * scale; returns the last register as it is (value * its scale)"""
    regs = [x]
    for s in steps:
        if s.kind == api.POLY_POWER:
            v = regs[s.a] * regs[s.b] / primes[s.mul_level]
            if s.c == api.POLY_TAIL_ONE:
                v = 2 * v - round(s.tail_const)
            elif s.c >= 0:
                v = 2 * v - regs[s.c]
        elif s.kind == api.POLY_LEAF:
            v = np.full_like(x, s.w0[0])
            for i in range(s.n_terms):
                v = v + s.w[i][0] * regs[s.term_reg[i]]
        else:
            q = regs[s.a]
            if s.rescale_first:
                q = q / primes[steps[s.a - 1].level]
            v = q * regs[s.b] + regs[s.c]
            if s.rescale_after:
                v = v / primes[s.level + 1]
        regs.append(v)
    return regs[-1]


def through(plan, primes, a, I):
    """one coefficient through the refresh; the result is read at the caller's scale"""
    pr = [float(p) for p in primes]
    x = plan.k1 * DELTA * a + pr[0] * I
    for f in range(plan.cts_pieces):
        x = x * plan.cts_scale[f] / pr[plan.cts_level - f]
    x = run_steps(plan.eval_mod.steps, pr, x)
    for g in range(plan.stc_pieces):
        x = x * plan.stc_scale[g] / pr[plan.stc_level - 1 - g]
    return x / DELTA


def f_of(a, rho):
    return rho / (2 * np.pi) * np.sin(2 * np.pi * a / rho)


@pytest.mark.parametrize("K", [12, 16])
def test_flat_primes_value_and_label(K):
    plan = hg.bootstrap_plan(FLAT, DELTA, 17, K=K)
    assert plan.k1 == 4 and (plan.cts_level, plan.eval_level, plan.stc_level, plan.out_level) == (17, 13, 5, 1)
    rho = FLAT[0] / (plan.k1 * DELTA)
    assert rho == 256.0
    assert abs(plan.out_scale / DELTA - 1) <= 1e-12
    assert abs(plan.cts_label[-1] / 2.0 ** 50 - 1) <= 1e-12 and plan.eval_in_scale == plan.cts_label[-1]
    rng = np.random.default_rng(K)
    a = np.concatenate([rng.uniform(-0.5, 0.5, 61), [-0.5, 0.0, 0.5]])
    worst, m_worst, cubic = 0.0, 0.0, 0.0
    for I in range(-(K - 1), K):
        got = through(plan, FLAT, a, float(I))
        eps = a / rho
        u = (I + eps) / K
        assert np.max(np.abs(u)) <= 1.0
        m_worst = max(m_worst, np.max(np.abs(model(K, 30, 3, u) - np.sin(2 * np.pi * eps) / (2 * np.pi))))
        worst = max(worst, np.max(np.abs(got - f_of(a, rho))))
        cubic = max(cubic, np.max(np.abs(f_of(a, rho) - a) - (2 * np.pi) ** 2 * np.abs(a) ** 3 / (6 * rho ** 2) * 1.01))
    print(f"K {K}: interpolant alone {m_worst:.3e} (x rho = {m_worst * rho:.3e}), refresh model against f(a) {worst:.3e}")
    assert worst <= m_worst * rho + 1e-12 * rho
    assert cubic <= 0


def test_k1_of_one_and_the_defaults():
    plan = hg.bootstrap_plan(FLAT, DELTA, 17, message_ratio=1024.0)
    assert plan.k1 == 1 and (plan.K, plan.sine_degree, plan.double_angle) == (16, 30, 3)  # EvalModConfig(level_start)
    assert abs(plan.out_scale / DELTA - 1) <= 1e-12
    a = np.linspace(-0.5, 0.5, 33)
    got = through(plan, FLAT, a, 3.0)
    assert np.max(np.abs(got - f_of(a, 1024.0))) <= 1e-6  # K = 16 at degree 30: the interpolant's 1.2e-9 times rho


@pytest.mark.parametrize("chain,k1", [(CHAIN_A, 4), (CHAIN_B, 4096)])
def test_real_primes_levels_and_scales(chain, k1):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *chain, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")][:c.Q_size]
    assert len(primes) == 18
    plan = hg.bootstrap_plan(primes, DELTA, 17, K=12)
    assert plan.k1 == k1
    assert (plan.cts_level, plan.cts_pieces, plan.eval_level, plan.stc_level, plan.stc_pieces, plan.out_level) == (17, 3, 13, 5, 3, 1)
    q0, S = float(primes[0]), float(primes[13])
    assert plan.raise_scale == q0 * 12 and plan.eval_target_scale == S
    label = plan.raise_scale
    for f in range(3):
        q = float(primes[17 - f])
        assert plan.cts_scale[f] == pytest.approx((S / (q0 * 12)) ** (1 / 3) * q, rel=1e-12)
        label = label * plan.cts_scale[f] / q
        assert plan.cts_label[f] == label
    assert label == pytest.approx(S, rel=1e-12) and plan.eval_in_scale == label
    em = plan.eval_mod
    assert em.level == 5 and em.scale == plan.eval_out_scale == pytest.approx(S, rel=1e-12)
    assert em.steps[0].level <= 13 and len(em.steps) > 3
    assert plan.stc_in_scale == pytest.approx(plan.eval_out_scale * k1 * DELTA / q0, rel=1e-15)
    label = plan.stc_in_scale
    for g in range(3):
        q = float(primes[4 - g])
        assert plan.stc_scale[g] == pytest.approx((DELTA / plan.stc_in_scale) ** (1 / 3) * q, rel=1e-12)
        assert 2.0 ** 30 < plan.stc_scale[g] < q
        label = label * plan.stc_scale[g] / q
        assert plan.stc_label[g] == label
    assert plan.out_scale == label and abs(label / DELTA - 1) <= 1e-12
    # the start levels may be stated; they must be the ones that follow
    same = hg.bootstrap_plan(primes, DELTA, 17, K=12, eval_level=13, stc_level=5)
    assert bytes(same.c) == bytes(plan.c)


def c_fill(primes=FLAT, plan=None, **kw):
    a = dict(scale=DELTA, message_ratio=256.0, K=12, sine_degree=30, double_angle=3, cts_level=17, cts_pieces=3, eval_level=-1,
             stc_level=-1, stc_pieces=3)
    a.update(kw)
    cfg = _lib.BootstrapConfig(*[a[n] for n, _ in _lib.BootstrapConfig._fields_])
    arr = (ctypes.c_uint64 * len(primes))(*primes)
    return _lib.load().hegpu_bootstrap_plan_fill(ctypes.byref(cfg), arr, len(primes), ctypes.byref(plan) if plan is not None else None)


REFUSALS = {
    "one level too few": dict(cts_level=15),  # 3 + 1 + 5 + 3 + 1 + 3 = 16 levels and a limb: cts_level >= 16
    "no such level": dict(cts_level=18),
    "K below 1": dict(K=0),
    "ratio times scale above q_0": dict(message_ratio=2048.0),
    "an infinite scale": dict(scale=float("inf")),
    "a scale that is not a number": dict(scale=float("nan")),
    "a scale of zero": dict(scale=0.0),
    "a ratio that is not a number": dict(message_ratio=float("nan")),
    "a negative ratio": dict(message_ratio=-256.0),
    "one CoeffToSlot piece": dict(cts_pieces=1),
    "six SlotToCoeff pieces": dict(stc_pieces=6),
    "EvalMod not where CoeffToSlot ends": dict(eval_level=12),
    "SlotToCoeff not where EvalMod ends": dict(stc_level=6),
    "a degree the evaluator refuses": dict(sine_degree=256),
    "nine double angles": dict(double_angle=9),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_leave_the_plan_untouched(why):
    plan = _lib.BootstrapPlan()
    ctypes.memset(ctypes.byref(plan), 0xA5, ctypes.sizeof(plan))
    before = bytes(plan)
    assert c_fill(plan=plan, **REFUSALS[why]) == hg.E_INVALID and bytes(plan) == before
    kw = dict(REFUSALS[why])
    with pytest.raises(hg.HEError) as e:
        hg.bootstrap_plan(FLAT, kw.pop("scale", DELTA), kw.pop("cts_level", 17), K=kw.pop("K", 12), **kw)
    assert e.value.code == hg.E_INVALID


def test_the_smallest_chain_that_fits_and_null_arguments():
    plan = _lib.BootstrapPlan()
    assert c_fill(plan=plan, cts_level=16, primes=FLAT[:17]) == 0 and plan.out_level == 0
    assert c_fill(plan=None) == hg.E_INVALID
    cfg = _lib.BootstrapConfig()
    assert _lib.load().hegpu_bootstrap_plan_fill(ctypes.byref(cfg), None, 18, ctypes.byref(plan)) == hg.E_INVALID
    assert _lib.load().hegpu_bootstrap_plan_fill(None, (ctypes.c_uint64 * 18)(*FLAT), 18, ctypes.byref(plan)) == hg.E_INVALID
