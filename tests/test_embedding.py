"""The CKKS encoding pinned by its definition at every degree the GPU encoder has a distinct FFT form for
(N = 2^12 .. 2^16): the oracle's plaintexts, brought to coefficients by the oracle's inverse NTT (itself pinned by the
ntt_by_definition goldens), CRT-composed in Python integers and evaluated at the slot roots by a plain FFT
(tests/embedding.py), give back message * scale -- slot order, conjugate placement and scaling included.  The
reference helpers are checked first: the CRT against small hand cases, the embedding against mpmath."""
import ctypes

import numpy as np
import pytest

from embedding import crt_centered, embed, embed_bound, evaluations, round_half_away, slot_index


def test_crt_centered_hand_cases():
    primes = [97, 193, 257]
    M = 97 * 193 * 257
    half = (M + 1) // 2
    xs = [0, 1, -1, 2, -2, 12345, -12345, half - 1, half, half + 1, M - 1]
    res = np.array([[x % q for x in xs] for q in primes], dtype=np.uint64)
    got = crt_centered(res, primes)
    want = [x if x % M < half else x % M - M for x in xs]
    assert got == want
    assert got[xs.index(half)] == half - M and got[xs.index(half - 1)] == half - 1  # (M+1)/2 is the first negative
    assert crt_centered(res, primes, positions=[3, 1]) == [want[3], want[1]]


def test_round_half_away():
    for v, k in ((0.5, 1), (-0.5, -1), (1.5, 2), (-2.5, -3), (0.49999999999999994, 0), (-0.0, 0), (2.0 ** 80, 2**80),
                 (-(2.0 ** 70 + 2.0 ** 18), -(2**70 + 2**18)), (5e-324, 0)):
        assert round_half_away(v) == k, v


def test_slot_roots_are_the_rotation_group():
    n = 64
    k, kc = slot_index(n)
    assert sorted(np.concatenate([k, kc]).tolist()) == list(range(n))  # every odd power once
    assert k[0] == 0 and k[1] == 2  # zeta^1, zeta^5
    assert kc[0] == n - 1          # zeta^(2N - 1) = conj(zeta)


@pytest.mark.parametrize("n", [2048, 4096])
def test_embed_matches_mpmath(n):
    import mpmath
    g = np.random.default_rng(n)
    coeffs = [int(v) for v in g.integers(-2**40, 2**40, n)]
    ev = evaluations(coeffs, n)
    k, kc = slot_index(n)
    mpmath.mp.dps = 40
    for j in (0, 1, 2, 7, n // 4, n // 2 - 1):
        for kk in (k[j], kc[j]):
            z = mpmath.exp(1j * mpmath.pi * (2 * int(kk) + 1) / n)
            want = mpmath.polyval(coeffs[::-1], z)
            assert abs(complex(want) - ev[kk]) < 1e-12 * np.sqrt(n) * 2**40, (j, kk)  # a wrong root: ~sqrt(N) 2^40


@pytest.fixture(scope="module", params=[12, 13, 14, 15, 16], ids=lambda p: f"N2^{p}")
def octx(request, oracle):
    n_power = request.param
    bits = (ctypes.c_int * 4)(60, 40, 40, 60)
    out = (ctypes.c_uint64 * 4)()
    assert oracle.lib().o_generate_primes(1 << n_power, bits, 4, out) == 0
    primes = [int(v) for v in out]
    return oracle.OracleContext(oracle.CKKS, n_power, primes, 3, 1), primes[:3]


def _coefficients(o, primes, plain):
    coeff = np.ascontiguousarray(plain, dtype=np.uint64).copy()
    o.ntt(coeff, o.Q, o.Q, inverse=True)
    return crt_centered(coeff, primes)


def _check_slots(n, coeffs, full, scale):
    slots, conj = embed(coeffs, n, conjugates=True)
    bound = embed_bound(n, full, scale)
    err = np.abs(slots - full * scale)
    assert np.all(err <= bound), f"slot error {err.max():.1f} > {bound[np.argmax(err - bound)]:.1f}"
    errc = np.abs(conj - np.conj(full) * scale)
    assert np.all(errc <= bound), f"conjugate slot error {errc.max():.1f}"


def test_oracle_slot_encodings_embed_to_message(octx):
    o, primes = octx
    n, slots = o.n, o.n // 2
    g = np.random.default_rng(o.n_power)
    scale = 2.0 ** 40
    x = g.uniform(-100, 100, slots)
    z = g.uniform(-50, 50, slots) + 1j * g.uniform(-50, 50, slots)
    for msg in (x, x[:slots // 2 + 3], x[:1]):
        full = np.zeros(slots, dtype=np.complex128)
        full[:len(msg)] = msg
        _check_slots(n, _coefficients(o, primes, o.ckks_encode(msg, scale)), full, scale)
    for msg in (z, z[:3], z[:slots - 1]):
        full = np.zeros(slots, dtype=np.complex128)
        full[:len(msg)] = msg
        _check_slots(n, _coefficients(o, primes, o.ckks_encode_ex(1, msg, scale)), full, scale)


def test_oracle_coefficient_encoding_is_the_rounded_polynomial(octx):
    o, primes = octx
    n = o.n
    g = np.random.default_rng(o.n_power + 100)
    scale = 2.0 ** 40
    m = g.uniform(-1000, 1000, n)
    for msg in (m, m[:5]):
        coeffs = _coefficients(o, primes, o.ckks_encode_ex(2, msg, scale))
        want = [round_half_away(float(v) * scale) for v in msg] + [0] * (n - len(msg))
        assert coeffs == want
