"""Inputs that drive the mod-down tail of the fused CKKS key switch to its extremes (shared by tests/test_gpu_fp_tail.py and
its instrumented run, tests/audit/run_tail_audit.py): the key-switched polynomial at the patterns of helpers.extreme_limbs
next to an all-(q - 1) key (the largest accumulators and T), the added ciphertext term 0 everywhere or q - 1 everywhere."""
import numpy as np

from helpers import extreme_limbs

PATTERNS = ("max", "max_coeff", "alt_coeff", "half_coeff")
TERMS = ("zero", "max")
C4_CHAIN = ([60] + [50] * 15, [60])


def max_key(primes, Q, Qp, n):
    """evaluation key [Q digits][2][Q' limbs][n], every residue q_j - 1"""
    return np.concatenate([np.full(n, primes[j] - 1, dtype=np.uint64) for _ in range(Q) for _c in range(2) for j in range(Qp)])


def _term(primes, l, n, term):
    return np.concatenate([np.full(n, primes[j] - 1 if term == "max" else 0, dtype=np.uint64) for j in range(l)])


def cases(c, primes, l, n, added_parts):
    """[(label, ciphertext)]: `added_parts` polynomials at the added term (relinearize: c0, c1; a rotation: c0), then the
    polynomial that is key-switched, one case per (pattern, term)"""
    out = []
    for i, pat in enumerate(PATTERNS):
        src = extreme_limbs(c, primes, range(l), n, pat, 3 + 31 * i)
        for term in TERMS:
            out.append(("%s/%s" % (pat, term), np.concatenate([_term(primes, l, n, term)] * added_parts + [src])))
    return out
