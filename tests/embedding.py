"""An independent reference for the CKKS encoding: exact CRT composition in Python integers and the
canonical embedding evaluated by a plain FFT, sharing nothing with the special FFT of the encoder.

A CKKS plaintext is the polynomial c(X) = sum_m c_m X^m mod X^N + 1; slot j holds c(zeta^(5^j mod 2N)) / scale with
zeta = exp(i pi / N), and the conjugate slot c(zeta^(-5^j mod 2N)) is its complex conjugate (the coefficients are
real).  `embed` evaluates c at every odd power of zeta with one inverse FFT of the twisted coefficients and picks
the slots out of it."""
from fractions import Fraction

import numpy as np


def crt_centered(residues, primes, positions=None):
    """residues: [l][N] (or flat l * N) coefficient-domain limbs mod primes[0..l-1].  The Python integers x in
    (-M/2, M/2] with x = residue mod q_i, at `positions` (all N by default).  A value is negative when its canonical
    representative is >= (M + 1) / 2 -- the reference's upper_half_threshold."""
    l = len(primes)
    r = np.asarray(residues, dtype=np.uint64).reshape(l, -1)
    idx = np.arange(r.shape[1]) if positions is None else np.asarray(positions)
    M = 1
    for q in primes:
        M *= int(q)
    half = (M + 1) // 2
    acc = np.zeros(len(idx), dtype=object)
    for i, q in enumerate(primes):
        q = int(q)
        mi = M // q
        w = mi * pow(mi % q, -1, q)  # = 1 mod q_i, 0 mod every other prime
        acc = acc + r[i, idx].astype(object) * w
    out = []
    for v in acc:
        v %= M
        out.append(v - M if v >= half else v)
    return out


def slot_index(n):
    """k(j) for the N/2 slots: slot j is evaluation k of `evaluations` (zeta^(2k + 1) = zeta^(5^j mod 2N))."""
    e = np.empty(n // 2, dtype=np.int64)
    p = 1
    for j in range(n // 2):
        e[j] = p
        p = p * 5 % (2 * n)
    return (e - 1) // 2, (2 * n - e - 1) // 2  # the slots, and their conjugates zeta^(-5^j)


def evaluations(coeffs, n):
    """c(zeta^(2k + 1)) for k < N: inverse DFT of the coefficients twisted by zeta^m (numpy, complex128)."""
    c = np.asarray([float(v) for v in coeffs], dtype=np.float64)
    assert len(c) == n
    twist = np.exp(1j * np.pi * np.arange(n) / n)
    return np.fft.ifft(c * twist) * n


def embed(coeffs, n, conjugates=False):
    """the N/2 slot values c(zeta^(5^j)) (times scale: divide by the scale to get the message); with
    conjugates=True also c(zeta^(-5^j)), which are their complex conjugates for real coefficients"""
    ev = evaluations(coeffs, n)
    k, kc = slot_index(n)
    return (ev[k], ev[kc]) if conjugates else ev[k]


def embed_bound(n, message, scale):
    """|embed(plaintext) - message * scale| allowed per slot: coefficient rounding (at most 1/2 per coefficient, summed
    over N coefficients of a root of unity: sqrt(N) size in practice) plus the error of the two FFTs, relative to
    the message"""
    return 8.0 * np.sqrt(n) + 2.0 ** -40 * np.abs(message) * scale


def round_half_away(v):
    """C round() of a double as an exact Python integer (halves away from zero)"""
    f = Fraction(v)
    a = abs(f)
    k = int(a + Fraction(1, 2))  # floor(|v| + 1/2), exact
    return -k if f < 0 else k


def compose_terms(x, primes, scale):
    """The terms the CRT-composing decoder adds for the centred integer x (kernel order, exact rationals): the
    canonical value a = x mod M in 64-bit words; for x >= 0 term j = a_j 2^(64 j) / scale, otherwise the word-wise
    signed difference (a_j - M_j) 2^(64 j) / scale."""
    M = 1
    for q in primes:
        M *= int(q)
    a = x % M
    terms = []
    for j in range(len(primes)):
        aj = (a >> (64 * j)) & (2**64 - 1)
        mj = (M >> (64 * j)) & (2**64 - 1)
        d = aj if x >= 0 else aj - mj
        terms.append(Fraction(d * 2 ** (64 * j)) / Fraction(scale))
    return terms
