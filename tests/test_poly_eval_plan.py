"""The evaluation plan of a polynomial on a CKKS ciphertext (heongpu_amd/csrc/poly_eval.cpp; host only, no GPU).

`restate` below is an independent restatement of the reference's schedule (HEOperator<CKKS>::evaluate_poly, gen_power,
evaluate_poly_recurse, evaluate_poly_from_polynomial_basis, Polynomial::split_coeffs; ckks/operator.cu:4292-4671,
:6633-6678) with the two departures poly_eval.hpp names: the depth is the bit length of the degree, and the conditional
rescale of q compares with target_scale / 2.  The plan must have the same steps; executed in plain complex arithmetic it
must give the polynomial.

On the execution check.  A register is held as value * scale; a product multiplies, a rescale divides by the prime, a
weight is divided by its scale ratio.  In the monomial basis every sum adds operands of exactly equal scale, so the
1e-9 bound holds with any primes.  In the Chebyshev basis the tail 2 T_a T_b - T_c subtracts a register of scale s_c
from a product of scale s_a s_b / q; with real primes the two differ by |q / 2^40 - 1| >= 2^-27, the approximation the
reference accepts, which is above 1e-9.  The algebra of the schedule is therefore checked with moduli equal to the scale
(2^40: the planner takes any integers), where that difference vanishes, and the structure is compared with real primes.
"""
import ctypes
import math

import numpy as np
import pytest

import heongpu_amd as hg
from heongpu_amd import _lib, api

DEGREES = [2, 3, 7, 12, 31, 32, 63]
BASES = [hg.MONOMIAL, hg.CHEBYSHEV]
SCALE = 2.0 ** 40
REAL_PRIMES = [(1 << 60) - 93] + [(1 << 40) + k * 8192 + 1 for k in (1, 4, 6, 9, 10, 13, 15, 21, 22, 24, 27)]
FLAT_PRIMES = [1 << 60] + [1 << 40] * 11


def coefficients(degree, seed, zeros=()):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, degree + 1) + 1j * rng.uniform(-1, 1, degree + 1)
    for z in zeros:
        if z <= degree:
            c[z] = 0
    return c


def round_away(v):
    """std::round: halves away from zero (Python's round() takes them to even)"""
    if abs(v) >= 2.0 ** 52:  # an integer already; v + 0.5 would round again
        return v
    return math.copysign(math.floor(abs(v) + 0.5), v)


def bit_length(v):
    return int(v).bit_length()


def optimal_split(log_degree):
    s = log_degree >> 1
    a = (1 << s) + (1 << (log_degree - s)) + log_degree - s - 3
    b = (1 << (s + 1)) + (1 << (log_degree - s - 1)) + log_degree - s - 4
    return s + 1 if a > b else s


def restate(basis, coeffs, level, scale, target_scale, primes, max_deg=None, lead=True):
    """-> list of dicts, one per step, registers numbered as the plan numbers them"""
    cheb = basis == hg.CHEBYSHEV
    regs = [(level, scale)]
    steps = []
    power = {1: 0}

    def prime(l):
        if l < 0 or l >= len(primes):
            raise ValueError("levels")
        return float(primes[l])

    def push(**kw):
        if kw["level"] < 0:
            raise ValueError("levels")
        kw["dst"] = len(regs)
        regs.append((kw["level"], kw["scale"]))
        steps.append(kw)
        return kw["dst"]

    def gen_power(p):
        if p in power:
            return
        c = 0
        if p & (p - 1) == 0:
            a = b = p // 2
        else:
            k = math.ceil(math.log2(p)) - 1
            a, b = (1 << k) - 1, p + 1 - (1 << k)
            if cheb:
                c = abs(a - b)
        gen_power(a)
        gen_power(b)
        if c:
            gen_power(c)
        (la, sa), (lb, sb) = regs[power[a]], regs[power[b]]
        ml = min(la, lb)
        if ml < 1:
            raise ValueError("levels")
        s = sa * sb
        s = s / prime(ml)
        lvl, tail = ml - 1, api.POLY_TAIL_NONE
        if cheb:
            tail = api.POLY_TAIL_ONE
            if c:
                tail = power[c]
                lvl = min(lvl, regs[tail][0])
        power[p] = push(kind=api.POLY_POWER, a=power[a], b=power[b], c=tail, level=lvl, mul_level=ml, scale=s)

    def split_coeffs(c, md, ld, split):
        degree = len(c) - 1
        md_r = split - 1 if md == degree else md - (degree - split + 1)
        r = list(c[:split])
        q = [c[split]] * (degree - split + 1)
        if not cheb:
            for i in range(split + 1, degree + 1):
                q[i - split] = c[i]
        else:
            for j, i in enumerate(range(split + 1, degree + 1), start=1):
                q[i - split] = 2.0 * c[i]
                r[split - j] = r[split - j] - c[i]
        return (q, md, ld), (r, md_r, False)

    def leaf(ts, tl, c):
        prime(tl)
        lvl = tl
        for i in range(1, len(c)):
            lvl = min(lvl, regs[power[i]][0])
        terms = []
        for i in range(1, len(c)):
            ratio = ts / regs[power[i]][1]
            w = complex(round_away(c[i].real * ratio), round_away(c[i].imag * ratio))
            if w != 0:
                terms.append((power[i], w))
        return push(kind=api.POLY_LEAF, level=lvl, scale=ts, terms=terms,
                    w0=complex(round_away(c[0].real * ts), round_away(c[0].imag * ts)))

    def recurse(tl, ts, pol, log_split):
        c, md, ld = pol
        degree, split = len(c) - 1, 1 << log_split
        if degree < split:
            if ld and log_split > 1 and degree > 0 and md % (1 << (log_split + 1)) > (1 << (log_split - 1)):
                return recurse(tl, ts, pol, math.ceil(math.log2(degree)) >> 1)
            if ld:
                ts = ts * prime(tl)
            return leaf(ts, tl, c)
        nxt = split
        while nxt < (degree >> 1) + 1:
            nxt <<= 1
        q, r = split_coeffs(c, md, ld, nxt)
        qi = prime(tl) if ld else prime(tl + 1)
        g = power[nxt]
        rq = recurse(tl + 1, ts * qi / regs[g][1], q, log_split)
        ql, qs = regs[rq]
        first = 0
        if qs >= target_scale / 2:
            if ql < 1:
                raise ValueError("levels")
            qs, ql, first = qs / prime(ql), ql - 1, 1
        ml = min(ql, regs[g][0])
        s = qs * regs[g][1]
        rr = recurse(ml, s, r, log_split)
        return push(kind=api.POLY_COMBINE, a=rq, b=g, c=rr, level=min(ml, regs[rr][0]), mul_level=ml, scale=s,
                    rescale_first=first)

    degree = len(coeffs) - 1
    log_degree = bit_length(degree)
    log_split = optimal_split(log_degree)
    for p in range((1 << log_split) - 1, 0, -1):
        gen_power(p)
    for i in range(log_split, log_degree):
        gen_power(1 << i)
    if level - log_degree + 1 < 0:
        raise ValueError("levels")
    recurse(level - log_degree + 1, target_scale, (list(coeffs), degree if max_deg is None else max_deg, lead), log_split)
    last = steps[-1]
    last["rescale_after"] = 0
    if last["scale"] / prime(last["level"]) >= target_scale / 2.0:
        if last["level"] < 1:
            raise ValueError("levels")
        last["scale"] = last["scale"] / prime(last["level"])
        last["level"] -= 1
        last["rescale_after"] = 1
    return steps


def min_level(degree):
    return bit_length(degree) + 1


CASES = [(b, d, lv) for b in BASES for d in DEGREES for lv in (min_level(d), min_level(d) + 1, 11)]


@pytest.mark.parametrize("basis,degree,level", CASES)
def test_plan_matches_the_restated_schedule(basis, degree, level):
    coeffs = coefficients(degree, 100 * degree + level, zeros=(0, 2, 5))
    plan = hg.poly_eval_plan(basis, coeffs, level, SCALE, SCALE, REAL_PRIMES)
    want = restate(basis, coeffs, level, SCALE, SCALE, REAL_PRIMES)
    assert len(plan.steps) == len(want)
    for got, w in zip(plan.steps, want):
        assert (got.kind, got.dst, got.level) == (w["kind"], w["dst"], w["level"])
        assert got.scale == pytest.approx(w["scale"], rel=1e-12)
        if w["kind"] == api.POLY_LEAF:
            assert got.n_terms == len(w["terms"])
            assert [got.term_reg[i] for i in range(got.n_terms)] == [r for r, _ in w["terms"]]
            # exactly round(c_i * (leaf_scale / scale_i)): the same doubles in the same order
            assert [complex(got.w[i][0], got.w[i][1]) for i in range(got.n_terms)] == [v for _, v in w["terms"]]
            assert complex(got.w0[0], got.w0[1]) == w["w0"]
            assert all(v != 0 for _, v in w["terms"])
        else:
            assert (got.a, got.b, got.c, got.mul_level) == (w["a"], w["b"], w["c"], w["mul_level"])
        if w["kind"] == api.POLY_COMBINE:
            assert got.rescale_first == w["rescale_first"]
        if w["kind"] == api.POLY_POWER and w["c"] == api.POLY_TAIL_ONE:
            assert got.tail_const == got.scale
        assert got.rescale_after == w.get("rescale_after", 0)
    assert (plan.level, plan.scale) == (plan.steps[-1].level, plan.steps[-1].scale)
    assert plan.scale == pytest.approx(SCALE, rel=1e-6)  # back at the target scale


def run_plan(plan, primes, x):
    """the plan in complex arithmetic on value * scale"""
    regs = [x * SCALE]
    for s in plan.steps:
        if s.kind == api.POLY_POWER:
            v = regs[s.a] * regs[s.b] / primes[s.mul_level]
            if s.c == api.POLY_TAIL_ONE:
                v = 2 * v - s.tail_const
            elif s.c >= 0:
                v = 2 * v - regs[s.c]
        elif s.kind == api.POLY_LEAF:
            v = np.full_like(x, complex(s.w0[0], s.w0[1]), dtype=np.complex128)
            for i in range(s.n_terms):
                v = v + complex(s.w[i][0], s.w[i][1]) * regs[s.term_reg[i]]
        else:
            q = regs[s.a]
            if s.rescale_first:  # by the prime at q's own level
                q = q / primes[plan.steps[s.a - 1].level]
            v = q * regs[s.b] + regs[s.c]
            if s.rescale_after:
                v = v / primes[s.level + 1]
        regs.append(v)
    return regs[-1] / plan.scale


@pytest.mark.parametrize("basis,degree,level", CASES)
def test_plan_computes_the_polynomial(basis, degree, level):
    coeffs = coefficients(degree, 7 * degree + level, zeros=(2,))
    # Chebyshev: moduli equal to the scale (module docstring); monomial: real primes
    primes = FLAT_PRIMES if basis == hg.CHEBYSHEV else REAL_PRIMES
    plan = hg.poly_eval_plan(basis, coeffs, level, SCALE, SCALE, primes)
    x = np.random.default_rng(degree).uniform(-1, 1, 64).astype(np.complex128)
    got = run_plan(plan, [float(p) for p in primes], x)
    want = (np.polynomial.chebyshev.chebval(x, coeffs) if basis == hg.CHEBYSHEV else np.polynomial.polynomial.polyval(x, coeffs))
    err = np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))
    print(f"basis {basis} degree {degree} level {level}: relative error {err:.3e}")
    assert err <= 1e-9


def c_plan_call(basis, coeffs, level, scale, target_scale, primes, max_deg=None, lead=1, fill_steps=None):
    lib = _lib.load()
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128))
    arr = (ctypes.c_uint64 * len(primes))(*primes)
    md = len(c) - 1 if max_deg is None else max_deg
    args = (basis, c.ctypes.data, len(c), md, lead, level, scale, target_scale, arr, len(primes))
    if fill_steps is None:
        count = ctypes.c_int(-7)
        return lib.hegpu_poly_eval_plan_size(*args, ctypes.byref(count)), count.value
    return lib.hegpu_poly_eval_plan_fill(*args, fill_steps, len(fill_steps)), None


REFUSALS = {
    "degree below 2": dict(coeffs=[1.0, 2.0]),
    "a leaf of more than 15 power terms": dict(coeffs=[1.0] * 257, level=11),
    "too few levels": dict(coeffs=[1.0] * 32, level=4),
    "a non-finite coefficient": dict(coeffs=[1.0, float("nan"), 1.0, 1.0]),
    "an infinite coefficient": dict(coeffs=[1.0, 1.0, float("inf"), 1.0]),
    "a non-finite scale": dict(coeffs=[1.0] * 4, scale=float("inf")),
    "a non-finite target scale": dict(coeffs=[1.0] * 4, target_scale=float("nan")),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(why):
    kw = dict(basis=hg.CHEBYSHEV, level=8, scale=SCALE, target_scale=SCALE, primes=REAL_PRIMES)
    kw.update(REFUSALS[why])
    rc, count = c_plan_call(**kw)
    assert rc == hg.E_INVALID and count == -7
    steps = (_lib.PolyStep * 4)()
    ctypes.memset(steps, 0xA5, ctypes.sizeof(steps))
    before = bytes(steps)
    rc, _ = c_plan_call(fill_steps=steps, **kw)
    assert rc == hg.E_INVALID and bytes(steps) == before
    with pytest.raises(hg.HEError) as e:
        hg.poly_eval_plan(kw["basis"], kw["coeffs"], kw["level"], kw["scale"], kw["target_scale"], kw["primes"])
    assert e.value.code == hg.E_INVALID


def test_fill_refuses_a_wrong_step_count():
    coeffs = coefficients(7, 1)
    rc, count = c_plan_call(hg.MONOMIAL, coeffs, 8, SCALE, SCALE, REAL_PRIMES)
    assert rc == 0 and count > 0
    steps = (_lib.PolyStep * (count + 1))()
    ctypes.memset(steps, 0xA5, ctypes.sizeof(steps))
    before = bytes(steps)
    rc, _ = c_plan_call(hg.MONOMIAL, coeffs, 8, SCALE, SCALE, REAL_PRIMES, fill_steps=steps)
    assert rc == hg.E_INVALID and bytes(steps) == before
