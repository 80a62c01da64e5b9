"""The fused FP64 row pass + key inner product with every quotient taken from the rounded product (fpmod.cuh fp_mul_nc
in ntt.hip ks_fp_row, ks_row_mac_fp_body and ks_tail_store_fp), bit for bit against the CPU oracle and against the same
call with every modulus on the integer butterflies (fp_ntt = 0).  The fused path is forced (fused_row_mac = 1).

  * chain {60, 50, 50, 50 | 60} at N = 2^12 and 2^13, two ciphertexts: the smallest degrees the fused row pass takes,
    both register rounds of ks_fp_row, ks_row_mac_fp_moddown on the Q slots;
  * the same chain at N = 2^16, two ciphertexts, with moddown_in_mac 1 (ks_row_mac_fp_moddown) and 0 (ks_row_mac_fp);
  * one ciphertext with the digits of a launch split in two (digit_split = 2: four digits is the fewest it takes), which
    runs the FP64 body of ks_row_mac_split;
  * a chain of primes just below 2^50 (from_primes): the largest moduli of the FP64 path, where every bound is tightest;
  * inputs: the extreme patterns of tests/tail_inputs.py (largest digits, all-(q - 1) key, added term 0 and q - 1) and one
    seeded random ciphertext and key; relinearize and one rotation.
(The product itself in exact arithmetic: tests/test_fp_model_quotient.py.)"""
import numpy as np
import pytest

import tail_inputs as ti
from helpers import backend_switches, synth_ct, synth_key

pytestmark = pytest.mark.gpu

CHAIN = ([60, 50, 50, 50], [60])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _is_prime(v):
    if v < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if v % p == 0:
            return v == p
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3 * 10^24
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


def ntt_primes_below(bits, count, n):
    """the `count` largest primes = 1 (mod 2n) below 2^bits, descending"""
    out, v = [], (1 << bits) + 1
    while len(out) < count:
        v -= 2 * n
        if _is_prime(v):
            out.append(v)
    assert all((1 << bits) - (1 << (bits - 8)) < p < (1 << bits) for p in out)
    return out


def make(hg, oracle, n_power, primes=None, **options):
    """(context with the FP64 path, context with fp_ntt = 0, oracle, primes, Q), the fused path forced in both"""
    n = 1 << n_power
    cs = []
    for fp in (1, 0):
        with backend_switches(HEGPU_FUSED_ROW_MAC=1, HEGPU_FP_NTT=fp, **{"HEGPU_" + k.upper(): v for k, v in options.items()}):
            if primes is None:
                c = hg.Context.from_bit_sizes(hg.CKKS, n, CHAIN[0], CHAIN[1], sec=hg.SEC_NONE)
            else:
                c = hg.Context.from_primes(hg.CKKS, n, primes, len(primes) - 1, 1)
        assert c.get_option("fused_row_mac") == 1 and c.get_option("fp_ntt") == fp
        for k, v in options.items():
            assert c.get_option(k) == v
        cs.append(c)
    got = [int(x) for x in cs[0].table("modulus")]
    assert got == [int(x) for x in cs[1].table("modulus")] and (primes is None or got == primes)
    Q = len(got) - 1
    for c in cs:
        c.upload()
    return cs[0], cs[1], oracle.OracleContext(oracle.CKKS, n_power, got, Q, 1), got, Q


def inputs(c, primes, l, n, parts):
    """[(label, ciphertext of `parts` added polynomials + the key-switched one, key)]: every extreme pattern with the
    added term 0 and q - 1 next to the all-(q - 1) key, then one seeded random ciphertext and key"""
    kmax = ti.max_key(primes, l, l + 1, n)
    out = [(label, x, kmax) for label, x in ti.cases(c, primes, l, n, parts)]
    assert len(out) == len(ti.PATTERNS) * len(ti.TERMS)
    out.append(("random", synth_ct(primes, range(l), parts + 1, n, 5), synth_key(primes, l, l + 1, n, 7)))
    return out


def launches(cases, batch):
    """the cases in launches of `batch` ciphertexts that share a key (the last of a key may be smaller; a lone random
    case is doubled so that every launch keeps the batch the shape is about)"""
    out = []
    for case in cases:
        if out and len(out[-1]) < batch and out[-1][0][2] is case[2]:
            out[-1].append(case)
        else:
            out.append([case])
    for g in out:
        while len(g) < batch:
            g.append(g[0])
    return out


def check_relinearize(hg, torch, c, c_int, o, l, n, cases, batch):
    for group in launches(cases, batch):
        key = group[0][2]
        dkey = hg.to_device(key)
        got = []
        for ctx in (c, c_int):
            d = hg.to_device(np.concatenate([x for _, x, _ in group]))
            ctx.ckks_relinearize_inplace(d, 3 * l * n, dkey, 0, len(group), ctx.workspace(hg.OP_CKKS_RELIN, 0, len(group)))
            torch.cuda.synchronize()
            got.append(hg.to_host(d).reshape(len(group), -1)[:, :2 * l * n])
        assert np.array_equal(got[0], got[1]), ("relinearize: FP64 path differs from fp_ntt = 0", [g[0] for g in group])
        for b, (label, x, _) in enumerate(group):
            want = o.ckks_relinearize(x.copy(), key, 0)
            assert np.array_equal(got[0][b], want[:2 * l * n]), ("relinearize", label)


def check_rotation(hg, torch, c, c_int, o, l, n, cases, batch, steps=1):
    g = hg.steps_to_galois_elt(steps, n, 5)
    for group in launches(cases, batch):
        key = group[0][2]
        dkey = hg.to_device(key)
        d = hg.to_device(np.concatenate([x for _, x, _ in group]))
        got = []
        for ctx in (c, c_int):
            rot = torch.empty(len(group) * 2 * l * n, dtype=torch.int64, device="cuda")
            ctx.ckks_apply_galois(d, 2 * l * n, rot, 2 * l * n, dkey, g, 0, len(group), ctx.workspace(hg.OP_CKKS_GALOIS, 0, len(group)))
            torch.cuda.synchronize()
            got.append(hg.to_host(rot).reshape(len(group), -1))
        assert np.array_equal(got[0], got[1]), ("rotation: FP64 path differs from fp_ntt = 0", [g_[0] for g_ in group])
        for b, (label, x, _) in enumerate(group):
            assert np.array_equal(got[0][b], o.ckks_apply_galois(x.copy(), key, g, 0)), ("rotation", label)


def run(hg, oracle, torch, n_power, batch, primes=None, **options):
    n = 1 << n_power
    c, c_int, o, primes, l = make(hg, oracle, n_power, primes=primes, **options)
    assert sum(q < 2 ** 50 for q in primes[:l]) >= 3  # the FP64 slots this file is about
    check_relinearize(hg, torch, c, c_int, o, l, n, inputs(c, primes, l, n, 2), batch)
    check_rotation(hg, torch, c, c_int, o, l, n, inputs(c, primes, l, n, 1), batch)


@pytest.mark.parametrize("n_power", [12, 13])
def test_smallest_degrees_two_ciphertexts(hg, oracle, torch, n_power):
    run(hg, oracle, torch, n_power, 2)


@pytest.mark.parametrize("moddown_in_mac", [1, 0])
def test_degree_2_16_two_ciphertexts(hg, oracle, torch, moddown_in_mac):
    run(hg, oracle, torch, 16, 2, moddown_in_mac=moddown_in_mac)


def test_one_ciphertext_split_launch(hg, oracle, torch):
    run(hg, oracle, torch, 12, 1, digit_split=2)


def test_primes_just_below_2_50(hg, oracle, torch):
    n_power = 12
    primes = ntt_primes_below(50, 5, 1 << n_power)
    assert all(q < 2 ** 50 for q in primes)
    run(hg, oracle, torch, n_power, 2, primes=primes)
