"""The fused CKKS key switch with the digits of the 60- and 61-bit moduli going into the 128-bit inner product
un-reduced (ntt.hip ks_row_digit's EXIT, decided per launch by ks_unreduced_exit in ops.cpp: keyswitch_ntt_mac), bit for
bit against the CPU oracle at the smallest shape that reaches the kernels: N = 2^12 with the fused path forced.

  * chains {60 | 60}, {60, 60 | 60}, {60, 50, 50 | 60} and {60, 50, 50, 50 | 60}: the P slot (ks_row_mac), the q_0 slot
    with its mod-down tail (ks_row_mac_moddown), all slots in ks_row_mac (moddown_in_mac = 0) and the integer tiles of
    ks_row_mac_split (digit_split = 2, which takes four digits or more: the four-prime chain);
  * inputs at the extremes: the key-switched polynomial at the patterns of tests/tail_inputs.py next to a key of all
    q - 1, the added term 0 and q - 1; the all-zero ciphertext; seeded random ciphertext and key;
  * relinearize and one rotation, batches of 2 (and 1);
  * both sides of the bound: 60-bit chains of 16, 17, 21, 22, 32 digits (exit bounds 16 q, 12 q, 12 q, 8 q, 8 q -- 32 is
    the most the flag accepts) and 33 (refused: the canonical end of before); 61-bit chains of 8 (accepted, 8 q) and 9
    digits (refused); a 61-bit modulus next to 60-bit ones in one launch; the same with digit_split = 2, where a
    workgroup sums half the digits and the bound moves accordingly (33 digits in ranges of 16 and 17).
The bound itself and the correction schedule: tests/test_int_mac_unreduced_model.py."""
import numpy as np
import pytest

import tail_inputs as ti
from helpers import backend_switches, synth_ct, synth_key

pytestmark = pytest.mark.gpu

N_POWER = 12
N = 1 << N_POWER


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


def ntt_primes_below(bits, count):
    """the `count` largest primes = 1 (mod 2N) below 2^bits, descending"""
    out, v = [], (1 << bits) - ((1 << bits) % (2 * N)) + 1
    while len(out) < count:
        v -= 2 * N
        if _is_prime(v):
            out.append(v)
    assert all((1 << (bits - 1)) < p < (1 << bits) for p in out)
    return out


def make(hg, oracle, primes=None, bits=None, Q=None, **options):
    with backend_switches(HEGPU_FUSED_ROW_MAC=1, **{"HEGPU_" + k.upper(): v for k, v in options.items()}):
        if primes is None:
            c = hg.Context.from_bit_sizes(hg.CKKS, N, bits[0], bits[1], sec=hg.SEC_NONE)
            Q = len(bits[0])
        else:
            c = hg.Context.from_primes(hg.CKKS, N, primes, Q, 1)
    assert c.get_option("fused_row_mac") == 1
    for k, v in options.items():
        assert c.get_option(k) == v
    primes = [int(x) for x in c.table("modulus")]
    assert len(primes) == Q + 1
    c.upload()
    return c, oracle.OracleContext(oracle.CKKS, N_POWER, primes, Q, 1), primes, Q


def inputs(c, primes, l, parts, patterns=ti.PATTERNS):
    """[(label, ciphertext of `parts` added polynomials + the key-switched one, key)]"""
    kmax = ti.max_key(primes, l, l + 1, N)
    out = [(label, x, kmax) for label, x in ti.cases(c, primes, l, N, parts) if label.split("/")[0] in patterns]
    out.append(("zero", np.zeros((parts + 1) * l * N, dtype=np.uint64), kmax))
    out.append(("random", synth_ct(primes, range(l), parts + 1, N, 5), synth_key(primes, l, l + 1, N, 7)))
    return out


def launches(cases, batch):
    """the cases in launches of up to `batch` ciphertexts that share a key"""
    out = []
    for case in cases:
        if out and len(out[-1]) < batch and out[-1][0][2] is case[2]:
            out[-1].append(case)
        else:
            out.append([case])
    assert sum(len(g) for g in out) == len(cases)
    return out


def check_relinearize(hg, torch, c, o, l, cases, batches=(2,)):
    for batch in batches:
        for group in launches(cases, batch):
            key = group[0][2]
            d = hg.to_device(np.concatenate([x for _, x, _ in group]))
            c.ckks_relinearize_inplace(d, 3 * l * N, hg.to_device(key), 0, len(group), c.workspace(hg.OP_CKKS_RELIN, 0, len(group)))
            torch.cuda.synchronize()
            got = hg.to_host(d).reshape(len(group), -1)
            for b, (label, x, _) in enumerate(group):
                want = o.ckks_relinearize(x.copy(), key, 0)
                assert np.array_equal(got[b][:2 * l * N], want[:2 * l * N]), ("relinearize", label, batch)


def check_rotation(hg, torch, c, o, l, cases, steps=1):
    g = hg.steps_to_galois_elt(steps, N, 5)
    for group in launches(cases, 2):
        key = group[0][2]
        d = hg.to_device(np.concatenate([x for _, x, _ in group]))
        rot = torch.empty(len(group) * 2 * l * N, dtype=torch.int64, device="cuda")
        c.ckks_apply_galois(d, 2 * l * N, rot, 2 * l * N, hg.to_device(key), g, 0, len(group), c.workspace(hg.OP_CKKS_GALOIS, 0, len(group)))
        torch.cuda.synchronize()
        got = hg.to_host(rot).reshape(len(group), -1)
        for b, (label, x, _) in enumerate(group):
            assert np.array_equal(got[b], o.ckks_apply_galois(x.copy(), key, g, 0)), ("rotation", label)


# (chain, options): digit_split = 2 splits only launches of four digits or more (ops.cpp: fused_digit_splits)
EXTREMES = [
    (([60], [60]), {}),
    (([60, 60], [60]), {}),
    (([60, 60], [60]), {"moddown_in_mac": 0}),
    (([60, 50, 50], [60]), {}),
    (([60, 50, 50], [60]), {"moddown_in_mac": 0}),
    (([60, 50, 50], [60]), {"digit_split": 2}),
    (([60, 50, 50, 50], [60]), {}),
    (([60, 50, 50, 50], [60]), {"digit_split": 2}),
]


def _ids(rows):
    return ["-".join(str(v) if not isinstance(v, dict) else ",".join("%s=%d" % kv for kv in v.items()) or "default" for v in r)
            .replace(" ", "") for r in rows]


@pytest.mark.parametrize("bits,options", EXTREMES, ids=_ids(EXTREMES))
def test_extremes_match_oracle(hg, oracle, torch, bits, options):
    c, o, primes, l = make(hg, oracle, bits=bits, **options)
    assert primes[0] >> 59 == 1 and primes[-1] >> 59 == 1  # q_0 and P on the correcting butterflies, room 16
    check_relinearize(hg, torch, c, o, l, inputs(c, primes, l, 2), batches=(2, 1) if not options else (2,))
    check_rotation(hg, torch, c, o, l, inputs(c, primes, l, 1))


# (modulus bits, digits, options): what ks_unreduced_exit gives the launch is in the comment
BOUND = [
    (60, 16, {}),                   # 16 q: the most digits that leave 16 q
    (60, 17, {}),                   # 12 q
    (60, 21, {}),                   # 12 q: the most
    (60, 22, {}),                   # 8 q
    (60, 32, {}),                   # 8 q: the most digits the flag accepts
    (60, 33, {}),                   # refused: canonical digits
    (61, 8, {}),                    # 8 q: the most for a 61-bit chain
    (61, 9, {}),                    # refused
    (60, 33, {"digit_split": 2}),   # ranges of 16 and 17 digits: judged by the 17, 12 q
    (61, 9, {"digit_split": 2}),    # ranges of 4 and 5: 8 q
    (61, 17, {"digit_split": 2}),   # ranges of 8 and 9: refused
]


@pytest.mark.parametrize("q_bits,digits,options", BOUND, ids=_ids(BOUND))
def test_both_sides_of_the_bound_match_oracle(hg, oracle, torch, q_bits, digits, options):
    c, o, primes, l = make(hg, oracle, primes=ntt_primes_below(q_bits, digits + 1), Q=digits, **options)
    assert l == digits
    cases = inputs(c, primes, l, 2, patterns=("max_coeff",))  # max_coeff / zero, / max, zero, random
    check_relinearize(hg, torch, c, o, l, cases)


def test_61_bit_modulus_next_to_60_bit_ones(hg, oracle, torch):
    """one launch, both rooms: the flag follows the 61-bit modulus, the 60-bit ones leave what it allows"""
    p60 = ntt_primes_below(60, 3)
    primes = [ntt_primes_below(61, 1)[0], p60[0], p60[1], p60[2]]
    c, o, primes, l = make(hg, oracle, primes=primes, Q=3)
    check_relinearize(hg, torch, c, o, l, inputs(c, primes, l, 2, patterns=("max_coeff", "alt_coeff")))
    check_rotation(hg, torch, c, o, l, inputs(c, primes, l, 1, patterns=("max_coeff",)))
