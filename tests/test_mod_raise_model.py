"""The modulus raise as a load transform, on Python integers (no GPU).

hegpu_ckks_mod_raise does not run a lifting kernel: its forward transform loads the q_0 limb through the mod-down's
first stage, ((v + half) mod q_0) mod q_j - half mod q_j.  With half = (q_0 + 1) / 2 that is the residue of the centred
representative the reference's mod_raise_kernel lifts (v - q_0 from v = q_0 >> 1 on); with the mod-down's own half,
(q_0 - 1) / 2, it would be wrong at exactly one value, v = (q_0 - 1) / 2, which the edge list holds.  The context's table
mod_raise_half_mod is checked against the same integers, and both entries refuse bad arguments before they need a device."""
import random

import pytest

import heongpu_amd as hg

N = 4096


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_of_bits(bits, skip=0):
    """the (skip + 1)-th prime below 2^bits that is 1 modulo 2N"""
    q = (1 << bits) - 2 * N + 1
    while True:
        if is_prime(q):
            if skip == 0:
                return q
            skip -= 1
        q -= 2 * N


def reference_residue(v, q0, qj):
    """mod_raise_kernel's word, made canonical (q_j -> 0)"""
    if v >= (q0 >> 1):
        return (qj - (q0 - v) % qj) % qj
    return v % qj


def load_transform(v, q0, qj, half):
    return ((v + half) % q0 % qj - half % qj) % qj


@pytest.mark.parametrize("q0_bits", [60, 50, 40])
def test_half_identity(q0_bits):
    q0 = prime_of_bits(q0_bits)
    h = (q0 - 1) // 2
    assert (q0 >> 1) == h
    rng = random.Random(q0_bits)
    values = [0, 1, h - 1, h, h + 1, q0 - 1] + [rng.randrange(q0) for _ in range(10000)]
    for t_bits in (30, 40, 50, 60, 61):
        qj = prime_of_bits(t_bits, skip=1)
        assert qj != q0
        values_j = values + [q0 - k * qj for k in (1, 2, 3) if k * qj < q0] + [k * qj for k in (1, 2, 3) if k * qj < q0]
        for v in values_j:
            assert load_transform(v, q0, qj, (q0 + 1) // 2) == reference_residue(v, q0, qj), (q0_bits, t_bits, v)
        # the mod-down's own half misses the reference's threshold by one value, and only by that one
        off = [v for v in values_j if load_transform(v, q0, qj, (q0 - 1) // 2) != reference_residue(v, q0, qj)]
        assert off == [h], (q0_bits, t_bits, off)


CHAINS = [([60, 40, 30, 50, 60], [60]), ([40, 60, 50, 36], [60]), ([50, 40], [50])]


@pytest.mark.parametrize("log_q,log_p", CHAINS)
def test_context_table(log_q, log_p):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(v) for v in c.table("modulus")]
    half = (primes[0] + 1) // 2
    assert [int(v) for v in c.table("mod_raise_half_mod")] == [half % q for q in primes[:len(log_q)]]
    for batch in (1, 3):
        for depth in range(len(log_q)):
            assert c.workspace_bytes(hg.OP_CKKS_MOD_RAISE, depth, batch) == 2 * N * 8 * batch
    bfv = hg.Context.from_default(hg.BFV, N, 1, 1032193)
    with pytest.raises(KeyError):
        bfv.table("mod_raise_half_mod")


def test_refusals_need_no_device():
    """addresses are plain integers: nothing is dereferenced, nothing is uploaded, before an argument is refused"""
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *CHAINS[0], sec=hg.SEC_NONE)
    Q = 5
    src, out, ws = 1 << 20, 1 << 24, 1 << 28
    wsb = 2 * N * 8

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID

    refused(lambda: c.mod_raise(None, 2 * N, out, 2 * Q * N, Q, 2, 1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, None, 2 * Q * N, Q, 2, 1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 2, 0, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 2, -1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, 0, 2, 1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q + 1, 2, 1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 0, 1, stream=0))
    refused(lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 4, 1, stream=0))
    refused(lambda: c.mod_raise(out + 8 * N, 2 * N, out, 2 * Q * N, Q, 2, 1, stream=0))            # inside the output
    refused(lambda: c.mod_raise(out - 8 * N, 2 * N, out, 2 * Q * N, Q, 2, 1, stream=0))            # its second part is
    refused(lambda: c.mod_raise(out + 8 * 4 * Q * N, 4 * Q * N, out, 4 * Q * N, Q, 2, 2, stream=0))  # item 0 in = item 1 out
    refused(lambda: c.ckks_mod_raise(None, 2 * N, out, 2 * Q * N, 0, 1, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, None, 2 * Q * N, 0, 1, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, None, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 0, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, -1, 1, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, Q, 1, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, ws, ws_bytes=wsb - 1, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 2, ws, ws_bytes=2 * wsb - 8, stream=0))
    refused(lambda: c.ckks_mod_raise(out + 8 * N, 2 * N, out, 2 * Q * N, 0, 1, ws, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, out + 8 * N, ws_bytes=wsb, stream=0))
    refused(lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, src + 8 * N, ws_bytes=wsb, stream=0))
    bfv = hg.Context.from_default(hg.BFV, N, 1, 1032193)
    refused(lambda: bfv.ckks_mod_raise(src, 2 * N, out, 2 * N, 0, 1, ws, ws_bytes=wsb, stream=0))
