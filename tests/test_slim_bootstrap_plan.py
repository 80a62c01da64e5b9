"""The plan of the slim, bit and gate refreshes (heongpu_amd/csrc/bootstrap_plan.cpp slim_bootstrap_plan; host only, no
GPU): every level and scale label between the input at level P_stc and the refreshed ciphertext.

  * the labels multiply through exactly: label_g = label_(g-1) * stc_scale[g] / q, the same for CoeffToSlot;
  * stc_label[last] * ratio / q_0 and cts_label[last] / eval_in_scale are within 1e-12 of 1 (a cube root and half a dozen
    products of doubles: a few 1e-16);
  * out_level = cts_level - P_cts - 1 - bit_length(degree) - r; out_scale = eval_out_scale / ratio for the arithmetic
    function and eval_out_scale for bit and gates;
  * one slot through the whole refresh in doubles on flat 2^50 primes (`through`, as tests/test_bootstrap_plan.py): the
    value read at out_scale is f(z) for slim and the truth table for bit and gates, to the interpolant's error;
  * refusals leave the plan untouched.
Chains: A and B of tests/test_gpu_bootstrap.py, the 24 x 41-bit chain of the reference's bit example (scale 2^41) and the
20 x 40-bit chain of its gate example (scale 2^40, q_0 = 3 * 2^40 to a few parts in 10^7)."""
import ctypes
import math

import numpy as np
import pytest

import heongpu_amd as hg
from heongpu_amd import _lib, api

N = 4096
FLAT = [1 << 50] * 18
CHAIN_A = ([50, 40, 40, 40, 40, 40] + [50] * 8 + [50] + [50] * 3, [60])
CHAIN_B = ([60, 40, 40, 40, 40, 40] + [60] * 8 + [56] + [56] * 3, [60])
CHAIN_BIT = ([42] + [41] * 23, [42, 42, 42])
GATE_Q = [3298535538689, 1099512938497, 1099515691009, 1099516870657, 1099521458177, 1099522375681, 1099523555329,
          1099525128193, 1099526176769, 1099529060353, 1099535220737, 1099536138241, 1099537580033, 1099538104321,
          1099540725761, 1099540856833, 1099543085057, 1099544002561, 1099544395777, 1099548327937]
TABLES = {"bit": [0, 1], "and": [0, 0, 1], "or": [0, 1, 1], "xor": [0, 1, 0], "nand": [1, 1, 0], "nor": [1, 0, 0],
          "xnor": [1, 0, 1]}


def primes_of(chain):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *chain, sec=hg.SEC_NONE)
    return [int(x) for x in c.table("modulus")][:c.Q_size]


def run_steps(steps, primes, x):  # tests/test_bootstrap_plan.py
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


def through(plan, primes, scale, z, I):
    """one real slot through the refresh: the number the ciphertext holds, read at the plan's out_scale"""
    pr = [float(p) for p in primes]
    x = scale * z
    for g in range(plan.stc_pieces):
        x = x * plan.stc_scale[g] / pr[plan.in_level - g]
    x = x + pr[0] * I  # the raise: t = (q_0 / ratio) z + q_0 I
    for f in range(plan.cts_pieces):
        x = x * plan.cts_scale[f] / pr[plan.cts_level - f]
    return run_steps(plan.trig.steps, pr, x) / plan.out_scale


def check_labels(plan, primes, scale, arithmetic, ratio):
    pr = [float(p) for p in primes]
    assert plan.in_level == plan.stc_pieces
    label = scale
    for g in range(plan.stc_pieces):
        q = pr[plan.in_level - g]
        assert plan.stc_scale[g] >= 1.0
        label = label * plan.stc_scale[g] / q
        assert plan.stc_label[g] == label
    assert abs(plan.stc_label[-1] * ratio / pr[0] - 1) <= 1e-12
    assert plan.raise_scale == pr[0] * plan.K
    label = plan.raise_scale
    for f in range(plan.cts_pieces):
        q = pr[plan.cts_level - f]
        assert plan.cts_scale[f] >= 1.0
        label = label * plan.cts_scale[f] / q
        assert plan.cts_label[f] == label
    assert plan.eval_level == plan.cts_level - plan.cts_pieces - 1
    assert plan.eval_in_scale == label and abs(plan.cts_label[-1] / plan.eval_in_scale - 1) <= 1e-12
    assert plan.eval_target_scale == pr[plan.eval_level] and abs(plan.eval_in_scale / plan.eval_target_scale - 1) <= 1e-12
    assert plan.out_level == plan.eval_level - int(plan.degree).bit_length() - plan.double_angle
    assert plan.trig.level == plan.out_level and plan.trig.scale == plan.eval_out_scale
    assert plan.eval_out_scale == pytest.approx(plan.eval_target_scale, rel=1e-12)
    assert plan.out_scale == (plan.eval_out_scale / ratio if arithmetic else plan.eval_out_scale)
    assert (plan.ratio, plan.K, plan.degree, plan.double_angle) == (ratio, 12, 30, 3)


CHAINS = {
    "A": (lambda: primes_of(CHAIN_A), 2.0 ** 40, 5),
    "B": (lambda: primes_of(CHAIN_B), 2.0 ** 40, 5),
    "bit_24x41": (lambda: primes_of(CHAIN_BIT), 2.0 ** 41, 11),
    "gate_20x40": (lambda: list(GATE_Q), 2.0 ** 40, 7),
}


@pytest.mark.parametrize("function", ["slim", "bit", "and", "xnor"])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_real_primes_levels_and_labels(chain, function):
    make, scale, out_level = CHAINS[chain]
    primes = make()
    plan = hg.slim_bootstrap_plan(primes, scale, len(primes) - 1, function)
    ratio = 256.0 if function == "slim" else hg.SLIM_FUNCTIONS[function][0]
    check_labels(plan, primes, scale, function == "slim", ratio)
    assert (plan.in_level, plan.cts_level, plan.out_level) == (3, len(primes) - 1, out_level)
    assert (plan.phase, plan.amplitude, plan.offset) == hg.SLIM_FUNCTIONS[function][1:]
    if chain == "bit_24x41" and function == "bit" or chain == "gate_20x40" and function in ("and", "xnor"):
        # the reference's own setting: q_0 is ratio * scale, the SlotToCoeff diagonals sit at the primes' own size
        for g in range(3):
            assert abs(plan.stc_scale[g] / primes[3 - g] - 1) < 1e-3


def test_other_piece_counts_and_a_caller_ratio():
    primes = primes_of(CHAIN_A)
    plan = hg.slim_bootstrap_plan(primes, 2.0 ** 40, 17, "slim", cts_pieces=4, stc_pieces=2, ratio=64.0)
    check_labels(plan, primes, 2.0 ** 40, True, 64.0)
    assert (plan.in_level, plan.eval_level, plan.out_level) == (2, 12, 4)
    custom = hg.slim_bootstrap_plan(primes, 2.0 ** 40, 17, (4.0, 0.125, 0.5, -0.25))
    check_labels(custom, primes, 2.0 ** 40, False, 4.0)
    assert custom.out_scale == custom.eval_out_scale and custom.offset == -0.25


def test_flat_primes_slim_value():
    scale, rho = 2.0 ** 40, 256.0
    plan = hg.slim_bootstrap_plan(FLAT, scale, 17, "slim")
    check_labels(plan, FLAT, scale, True, rho)
    z = np.concatenate([np.random.default_rng(3).uniform(-0.5, 0.5, 61), [-0.5, 0.0, 0.5]])
    worst = 0.0
    for I in range(-11, 12):
        got = through(plan, FLAT, scale, z, float(I))
        worst = max(worst, np.max(np.abs(got - rho / (2 * np.pi) * np.sin(2 * np.pi * z / rho))))
    print(f"slim, flat primes: refresh model against f(z) {worst:.3e}")
    assert worst <= 1.7e-13 * rho + 1e-12 * rho  # the interpolant's own error and the rounded weights, times rho


@pytest.mark.parametrize("function", sorted(TABLES))
def test_flat_primes_truth_tables(function):
    scale = 2.0 ** 40
    plan = hg.slim_bootstrap_plan(FLAT, scale, 17, function)
    ratio = plan.ratio
    check_labels(plan, FLAT, scale, False, ratio)
    s = np.arange(len(TABLES[function]), dtype=np.float64)
    worst = 0.0
    for I in range(-11, 12):
        got = through(plan, FLAT, scale, s, float(I))
        worst = max(worst, np.max(np.abs(got - np.array(TABLES[function], dtype=np.float64))))
    print(f"{function}, flat primes: refresh model against the truth table {worst:.3e}")
    assert worst <= 1e-9


def c_fill(primes=FLAT, plan=None, **kw):
    a = dict(scale=2.0 ** 40, ratio=256.0, phase=0.25, amplitude=1 / (2 * math.pi), offset=0.0, K=12, degree=30, double_angle=3,
             cts_level=17, cts_pieces=3, stc_pieces=3, arithmetic=1, reserved=0)
    a.update(kw)
    cfg = _lib.SlimBootstrapConfig(*[a[n] for n, _ in _lib.SlimBootstrapConfig._fields_])
    arr = (ctypes.c_uint64 * len(primes))(*primes)
    return _lib.load().hegpu_slim_bootstrap_plan_fill(ctypes.byref(cfg), arr, len(primes),
                                                      ctypes.byref(plan) if plan is not None else None)


REFUSALS = {
    "one level too few": dict(cts_level=11),  # 3 + 1 + 5 + 3 = 12 levels and a limb: cts_level >= 12
    "no such level": dict(cts_level=18),
    "a chain shorter than SlotToCoeff": dict(primes=FLAT[:3], cts_level=2),
    "K below 1": dict(K=0),
    "a ratio below 2": dict(ratio=1.5),
    "a ratio that is not a number": dict(ratio=float("nan")),
    "an infinite ratio": dict(ratio=float("inf")),
    "an infinite scale": dict(scale=float("inf")),
    "a scale of zero": dict(scale=0.0),
    "one CoeffToSlot piece": dict(cts_pieces=1),
    "six SlotToCoeff pieces": dict(stc_pieces=6),
    "a SlotToCoeff factor's scale below one": dict(scale=2.0 ** 60, ratio=2.0 ** 170),
    "a degree the evaluator refuses": dict(degree=256),
    "nine double angles": dict(double_angle=9),
    "an amplitude of zero": dict(amplitude=0.0),
    "a phase that is not a number": dict(phase=float("nan")),
    "an infinite offset": dict(offset=float("inf")),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_leave_the_plan_untouched(why):
    plan = _lib.SlimBootstrapPlan()
    ctypes.memset(ctypes.byref(plan), 0xA5, ctypes.sizeof(plan))
    before = bytes(plan)
    assert c_fill(plan=plan, **REFUSALS[why]) == hg.E_INVALID and bytes(plan) == before


def test_python_refusals_and_the_smallest_chain():
    with pytest.raises(hg.HEError) as e:
        hg.slim_bootstrap_plan(FLAT, 2.0 ** 40, 11)
    assert e.value.code == hg.E_INVALID
    with pytest.raises(hg.HEError):
        hg.slim_bootstrap_plan(FLAT, 2.0 ** 40, 17, "slim", ratio=1.0)
    plan = _lib.SlimBootstrapPlan()
    assert c_fill(plan=plan, cts_level=12, primes=FLAT[:13]) == 0 and plan.out_level == 0 and plan.in_level == 3
    assert c_fill(plan=None) == hg.E_INVALID
    cfg = _lib.SlimBootstrapConfig()
    assert _lib.load().hegpu_slim_bootstrap_plan_fill(ctypes.byref(cfg), None, 18, ctypes.byref(plan)) == hg.E_INVALID
    assert _lib.load().hegpu_slim_bootstrap_plan_fill(None, (ctypes.c_uint64 * 18)(*FLAT), 18, ctypes.byref(plan)) == hg.E_INVALID
