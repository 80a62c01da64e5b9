"""The cosine with a phase, an amplitude and an offset as a plan (heongpu_amd/csrc/poly_eval.cpp eval_trig_plan; host only,
no GPU): alpha + A cos(2 pi (K u - phi)), the one function family of the slim, bit and gate refreshes.

  * (1/4, 1 / 2 pi, 0) is eval_mod_plan, field for field (the bytes of every step).
  * The plan interpreted in doubles (`run_plan`, the model of tests/test_eval_mod_plan.py: flat 2^50 primes, K = 12,
    degree 30, r = 0 and 3) gives the truth table of the bit refresh and of all six gates at every admissible integer I
    (|I| <= 11) and every clean input s in {0, 1, 2} (b in {0, 1}): |value - table| <= 1e-9.  That is the interpolant's own
    1.7e-13 times at most 2 pi, with room for the rounding of doubles; the figures are printed.
    Degree 30 cannot resolve cos(2 pi 12 u) without double angles (it takes a degree above 2 pi K = 75): at r = 0 the numpy
    model alone is off by 0.7 .. 1.4 (printed), and the bound is four times the model's figure; there the plan is held to
    the model instead, to 1e-9, which is what shows that the offset sits in Chebyshev coefficient 0.
  * The truth tables themselves, in exact trigonometry, at s = 0, 1, 2.
  * Refusals: what eval_mod_plan refuses, an amplitude <= 0, a non-finite phase, amplitude or offset."""
import ctypes
import math

import numpy as np
import pytest

import heongpu_amd as hg
from heongpu_amd import _lib, api

SCALE = 2.0 ** 50
FLAT_PRIMES = [1 << 50] * 13
REAL_PRIMES = [(1 << 50) + k * 8192 + 1 for k in (3, 4, 7, 9, 12, 16, 18, 19, 21, 22, 24, 27, 31)]
K, DEGREE, LEVEL = 12, 30, 12

TABLES = {  # the value at s = a + b = 0, 1, 2 (bit: b = 0, 1)
    "bit": [0, 1],
    "and": [0, 0, 1],
    "or": [0, 1, 1],
    "xor": [0, 1, 0],
    "nand": [1, 1, 0],
    "nor": [1, 0, 0],
    "xnor": [1, 0, 1],
}


def run_plan(plan, primes, u, scale):  # tests/test_eval_mod_plan.py
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


def model(phase, amplitude, offset, r, u):
    c = amplitude ** (1.0 / 2 ** r)
    coeffs = np.polynomial.chebyshev.chebinterpolate(lambda x: c * np.cos(2 * np.pi * (K * x - phase) / 2 ** r), DEGREE)
    y = np.polynomial.chebyshev.chebval(u, coeffs)
    for i in range(r):
        y = 2 * y * y - c ** (2 ** (i + 1))
    return y + offset


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("primes", [FLAT_PRIMES, REAL_PRIMES], ids=["flat", "real"])
def test_the_eval_mod_plan_is_the_special_case(primes, r):
    want = hg.eval_mod_plan(6, DEGREE, r, LEVEL, SCALE, 2.0 ** 48, primes)
    got = api.eval_trig_plan(6, DEGREE, r, 0.25, 1.0 / (2.0 * math.pi), 0.0, LEVEL, SCALE, 2.0 ** 48, primes)
    assert len(got.steps) == len(want.steps)
    assert bytes(got.steps) == bytes(want.steps)
    assert (got.level, got.scale, got.out_limbs) == (want.level, want.scale, want.out_limbs)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_family_in_exact_trigonometry(name):
    ratio, phase, amplitude, offset = hg.SLIM_FUNCTIONS[name]
    for s, want in enumerate(TABLES[name]):
        assert offset + amplitude * math.cos(2 * math.pi * (s / ratio - phase)) == pytest.approx(want, abs=1e-15)


@pytest.mark.parametrize("r", [0, 3])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_truth_tables_at_every_overflow(name, r):
    ratio, phase, amplitude, offset = hg.SLIM_FUNCTIONS[name]
    plan = api.eval_trig_plan(K, DEGREE, r, phase, amplitude, offset, LEVEL, SCALE, SCALE, FLAT_PRIMES)
    assert plan.level == LEVEL - 5 - r
    us, want = [], []
    for I in range(-(K - 1), K):
        for s, value in enumerate(TABLES[name]):
            us.append((I + s / ratio) / K)
            want.append(value)
    u, want = np.array(us), np.array(want, dtype=np.float64)
    assert len(u) == (2 * K - 1) * len(TABLES[name]) and np.max(np.abs(u)) <= 1.0
    m = model(phase, amplitude, offset, r, u)
    got = run_plan(plan, [float(p) for p in FLAT_PRIMES], u, SCALE)
    m_err, err, apart = np.max(np.abs(m - want)), np.max(np.abs(got - want)), np.max(np.abs(got - m))
    bound = 1e-9 if m_err <= 1e-9 else 4 * m_err
    print(f"{name} r = {r}: numpy model alone {m_err:.3e}, the plan in doubles {err:.3e} (bound {bound:.3e}), plan against "
          f"model {apart:.3e}")
    assert err <= bound
    assert apart <= 1e-9  # whatever the interpolant resolves, the plan computes it (r = 0: the offset in coefficient 0)
    if r:
        last = plan.steps[len(plan.steps) - 1]
        assert last.c == api.POLY_TAIL_ONE and last.tail_const == pytest.approx((amplitude - offset) * last.scale, abs=last.scale * 1e-15)
        assert round(last.tail_const) >= 0 and (round(last.tail_const) == 0) == (name in ("bit", "or", "nand", "xnor"))


def test_a_negative_tail_constant_is_a_plan():
    plan = api.eval_trig_plan(K, DEGREE, 3, 0.5, 0.5, 0.75, LEVEL, SCALE, SCALE, FLAT_PRIMES)
    last = plan.steps[len(plan.steps) - 1]
    assert last.tail_const == pytest.approx(-0.25 * last.scale, rel=1e-14) and round(last.tail_const) < 0
    u = np.array([0.0, 1.0 / (2 * K), -3.0 / K])
    got = run_plan(plan, [float(p) for p in FLAT_PRIMES], u, SCALE)
    assert np.max(np.abs(got - np.array([0.25, 1.25, 0.25]))) <= 1e-9


def c_call(K=K, degree=DEGREE, r=3, phase=0.5, amplitude=0.5, offset=0.5, level=LEVEL, scale=SCALE, target=SCALE,
           primes=REAL_PRIMES, fill_steps=None):
    lib = _lib.load()
    arr = (ctypes.c_uint64 * len(primes))(*primes)
    args = (K, degree, r, phase, amplitude, offset, level, scale, target, arr, len(primes))
    if fill_steps is None:
        count = ctypes.c_int(-7)
        return lib.hegpu_eval_trig_plan_size(*args, ctypes.byref(count)), count.value
    return lib.hegpu_eval_trig_plan_fill(*args, fill_steps, len(fill_steps)), None


REFUSALS = {
    "K below 1": dict(K=0),
    "negative double angle": dict(r=-1),
    "double angle above 8": dict(r=9),
    "degree below 2": dict(degree=1),
    "degree above 255": dict(degree=256),
    "too few levels": dict(level=7),
    "no such level": dict(level=13),
    "an infinite scale": dict(scale=float("inf")),
    "a scale of zero": dict(scale=0.0),
    "a target scale that is not a number": dict(target=float("nan")),
    "an amplitude of zero": dict(amplitude=0.0),
    "a negative amplitude": dict(amplitude=-0.5),
    "an infinite amplitude": dict(amplitude=float("inf")),
    "an amplitude that is not a number": dict(amplitude=float("nan")),
    "a phase that is not a number": dict(phase=float("nan")),
    "an infinite phase": dict(phase=float("-inf")),
    "an offset that is not a number": dict(offset=float("nan")),
    "an infinite offset": dict(offset=float("inf")),
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
    a = dict(K=K, degree=DEGREE, r=3, phase=0.5, amplitude=0.5, offset=0.5, level=LEVEL, scale=SCALE, target=SCALE)
    a.update(kw)
    with pytest.raises(hg.HEError) as e:
        api.eval_trig_plan(a["K"], a["degree"], a["r"], a["phase"], a["amplitude"], a["offset"], a["level"], a["scale"],
                           a["target"], REAL_PRIMES)
    assert e.value.code == hg.E_INVALID


def test_fill_wants_the_size_that_size_gives():
    rc, count = c_call()
    assert rc == 0 and count > 3
    steps = (_lib.PolyStep * (count - 1))()
    ctypes.memset(steps, 0xA5, ctypes.sizeof(steps))
    before = bytes(steps)
    rc, _ = c_call(fill_steps=steps)
    assert rc == hg.E_INVALID and bytes(steps) == before
    steps = (_lib.PolyStep * count)()
    rc, _ = c_call(fill_steps=steps)
    assert rc == 0 and steps[count - 1].dst == count
    lib = _lib.load()
    assert lib.hegpu_eval_trig_plan_size(K, DEGREE, 3, 0.5, 0.5, 0.5, LEVEL, SCALE, SCALE, None, 13,
                                         ctypes.byref(ctypes.c_int(0))) == hg.E_INVALID
