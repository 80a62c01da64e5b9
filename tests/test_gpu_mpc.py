"""N-out-of-N multiparty protocol through the C ABI (hegpu_mpc_*): collective public, relinearisation and Galois keys
and collective decryption, for k = 1, 2, 3, 5 parties.

No new oracle is needed: a collective key is a key under s = sum of the parties' s_i with the layout of the
single-party key, so it is correct iff the existing pipeline, given that s, decrypts what it should.  The sums are
exact and checked exactly; everything that carries fresh noise is checked against bounds derived from the samplers:
every error is a rounded Gaussian clipped at 6 sigma = 19.2 and every secret (s_i, u_i) is ternary, hence B = 20 per
error term.

  * collective public key:  pk[0] + pk[1] * s = -(sum e_i), at most k * B per coefficient.
  * collective decryption:  merge - (c0 + c1 * s) = sum e_i, at most k * B per coefficient.
  * collective relinearisation / Galois keys go through the evaluator with the margins of the single-party test
    (tests/test_gpu_keygen.py): 2^16 fresh, scale^2 / 2^8 after multiply + relinearize, scale / 2^8 after a rotation.
    Key noise of the collective relinearisation key per digit: s*e0 + (u - s)*e1 + e2 + e3 summed over the parties,
    i.e. at most k^2 * N * B (s*e0) + 2 * k^2 * N * B ((u - s)*e1) + 2 * k * B, against N * B for one party; the key
    switch divides it by P (>= 2^50) after multiplying by a digit below 2^50 (method I) or 2^72 against P = 2^74
    (method II), so at k = 5, N = 4096 it adds at most 3 * 25 * 4096 * 20 * l = 2^25 to a result whose margin is
    2^52 (scale^2 / 2^8) resp. 2^22 for the rotation, where the Galois key's noise is only k * N * B = 2^19 per digit.
"""
import ctypes

import numpy as np
import pytest

from he_math import RLWE, negacyclic_mul

pytestmark = pytest.mark.gpu

B = 20  # > 6 sigma = 19.2, the clip of every error sample (include/hegpu.h)
PARTIES = [1, 2, 3, 5]
CKKS_SETS = {"method_I": ([50, 30, 30, 30], [50]), "method_II": ([36, 36, 36], [37, 37])}
N = 4096
CRS_SEED = 9001


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _ckks(hg, oracle, name):
    log_q, log_p = CKKS_SETS[name]
    c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
    c.upload()
    return c, o, primes


def _bfv(hg, oracle):
    t = 1032193
    c = hg.Context.from_default(hg.BFV, N, 1, t)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, t)
    c.upload()
    return c, o, primes, t


def _limbs(t, hg, rows):
    return hg.to_host(t).reshape(-1, rows, N)


def _sum_mod(arrays, primes, rows):
    """limb-wise modular sum of [*][rows][N] arrays (q < 2^61 and at most 10 terms: no uint64 overflow)"""
    acc = np.zeros_like(arrays[0]).reshape(-1, rows, N)
    q = np.array(primes[:rows], dtype=np.uint64).reshape(1, rows, 1)
    for a in arrays:
        acc = (acc + a.reshape(-1, rows, N)) % q
    return acc


def _mul_mod(a, b, primes):
    """[rows][N] * [rows][N] limb-wise with Python integers"""
    return np.stack([np.array((a[j].astype(object) * b[j].astype(object)) % primes[j], dtype=np.uint64)
                     for j in range(a.shape[0])])


def _centred_limbs(rns, primes):
    """centred representative of a small polynomial from each limb; every limb must give the same one"""
    first = None
    for j in range(rns.shape[0]):
        q = primes[j]
        v = np.array([int(x) if int(x) <= q // 2 else int(x) - q for x in rns[j]], dtype=np.int64)
        if first is None:
            first = v
        assert np.array_equal(v, first), "the limbs disagree: not a small polynomial"
    return first


class Parties:
    """k parties with their secrets and generators; every party holds a crs generator of its own with the common seed"""

    def __init__(self, hg, c, k, crs_seed=CRS_SEED, rng_base=100):
        self.hg, self.c, self.k = hg, c, k
        self.rng = [hg.Rng(rng_base + i) for i in range(k)]
        self.crs = [hg.Rng(crs_seed) for _ in range(k)]
        self.sk = [c.generate_secret_key(self.rng[i]) for i in range(k)]

    def sum_secret(self, primes):
        Qp = self.c.Q_prime_size
        return _sum_mod([self.hg.to_host(s) for s in self.sk], primes, Qp).reshape(Qp, N)

    def public_key(self):
        c = self.c
        self.pk_shares = [c.mpc_public_key_share(self.crs[i], self.rng[i], self.sk[i]) for i in range(self.k)]
        return c.mpc_accumulate(self.pk_shares, self.hg.MPC_PUBLIC_KEY)

    def relin_key(self):
        c, k = self.c, self.k
        r1 = [c.mpc_relin_key_share_round1(self.crs[i], self.rng[i], self.sk[i]) for i in range(k)]
        self.u = [x[0] for x in r1]
        self.r1_shares = [x[1] for x in r1]
        self.r1_sum = c.mpc_accumulate(self.r1_shares, self.hg.MPC_RELIN_ROUND1)
        self.r2_shares = [c.mpc_relin_key_share_round2(self.rng[i], self.sk[i], self.u[i], self.r1_sum) for i in range(k)]
        return c.mpc_relin_key_finish(self.r2_shares, self.r1_sum)

    def galois_key(self, elt):
        c = self.c
        self.gk_shares = [c.mpc_galois_key_share(self.crs[i], self.rng[i], self.sk[i], elt) for i in range(self.k)]
        return c.mpc_accumulate(self.gk_shares, self.hg.MPC_GALOIS_KEY)

    def ckks_decrypt(self, ct, stride, depth=0, batch=1):
        shares = [self.c.mpc_ckks_decrypt_share(self.rng[i], ct, stride, self.sk[i], depth, batch) for i in range(self.k)]
        return self.c.mpc_ckks_decrypt_merge(ct, stride, shares, depth, batch), shares

    def bfv_decrypt(self, ct, stride, batch=1):
        shares = [self.c.mpc_bfv_decrypt_share(self.rng[i], ct, stride, self.sk[i], batch) for i in range(self.k)]
        return self.c.mpc_bfv_decrypt_merge(ct, stride, shares, batch), shares


@pytest.mark.parametrize("k", PARTIES)
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_collective_keys_are_exact_sums_with_bounded_noise(hg, oracle, torch, name, k):
    c, o, primes = _ckks(hg, oracle, name)
    Qp, d = c.Q_prime_size, c.switch_key_digits()
    he = RLWE(o, seed=1)
    p = Parties(hg, c, k)
    s = p.sum_secret(primes)
    # ---- public key: exact sum, the common a, and pk[0] + pk[1] * s = -(sum of the parties' errors)
    pk = _limbs(p.public_key(), hg, Qp)
    shares = [_limbs(x, hg, Qp) for x in p.pk_shares]
    assert np.array_equal(pk[0], _sum_mod([x[0] for x in shares], primes, Qp)[0]), "pk[0] = sum of the shares"
    for x in shares:
        assert np.array_equal(x[1], pk[1]), "pk[1] = the common a"
    noise = _sum_mod([pk[0], _mul_mod(pk[1], s, primes)], primes, Qp)[0]
    e = _centred_limbs(he.ntt_limbs(noise, list(range(Qp)), inverse=True), primes)
    print(f"{name} k={k}: max |pk noise| = {np.abs(e).max()} (bound {k * B})")
    assert np.abs(e).max() <= k * B
    # ---- relinearisation key: both round-1 parts summed; rk[0] = sum of both round-2 parts, rk[1] = h1
    rk = _limbs(p.relin_key(), hg, Qp).reshape(d, 2, Qp, N)
    r1 = _sum_mod([hg.to_host(x) for x in p.r1_shares], primes, Qp).reshape(d, 2, Qp, N)
    assert np.array_equal(_limbs(p.r1_sum, hg, Qp).reshape(d, 2, Qp, N), r1), "round-1 sum"
    r2 = [hg.to_host(x).reshape(d, 2, Qp, N) for x in p.r2_shares]
    want0 = _sum_mod([x[:, 0] for x in r2] + [x[:, 1] for x in r2], primes, Qp).reshape(d, Qp, N)
    assert np.array_equal(rk[:, 0], want0), "rk[0] = sum_i (share2_i[0] + share2_i[1])"
    assert np.array_equal(rk[:, 1], r1[:, 1]), "rk[1] = h1"
    # ---- Galois key
    gal = hg.steps_to_galois_elt(1, N, 5)
    gk = _limbs(p.galois_key(gal), hg, Qp).reshape(d, 2, Qp, N)
    gs = [hg.to_host(x).reshape(d, 2, Qp, N) for x in p.gk_shares]
    assert np.array_equal(gk[:, 0], _sum_mod([x[:, 0] for x in gs], primes, Qp).reshape(d, Qp, N)), "gk[0]"
    for x in gs:
        assert np.array_equal(x[:, 1], gk[:, 1]), "gk[1] = the common a_d"


_messages = {}


def _ckks_messages():
    if not _messages:
        g = np.random.default_rng(12)
        m1, m2 = g.integers(-8, 9, N), g.integers(-8, 9, N)
        _messages.update(m1=m1, m2=m2, prod=negacyclic_mul(m1, m2))
    return _messages["m1"], _messages["m2"], _messages["prod"]


@pytest.mark.parametrize("k", PARTIES)
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_ckks_evaluator_runs_on_collective_keys(hg, oracle, torch, name, k):
    """encrypt under the collective pk, multiply, relinearize with the collective rk, rescale, rotate with the
    collective gk; every result is opened by collective decryption (shares + merge), never with s -- s is only used to
    measure the noise the shares add.  Margins: the module docstring."""
    c, o, primes = _ckks(hg, oracle, name)
    Q, n = c.Q_size, N
    he = RLWE(o, seed=1)
    p = Parties(hg, c, k)
    pk, rk = p.public_key(), p.relin_key()
    gal = hg.steps_to_galois_elt(1, n, 5)
    gk = p.galois_key(gal)
    s = hg.to_device(p.sum_secret(primes).reshape(-1))
    enc = hg.Rng(77)
    scale = 1 << 30
    m1, m2, prod = _ckks_messages()
    p1 = he.to_ntt([int(v) * scale for v in m1], range(Q)).reshape(-1)
    p2 = he.to_ntt([int(v) * scale for v in m2], range(Q)).reshape(-1)
    ct1 = c.ckks_encrypt(enc, pk, hg.to_device(p1))
    ct2 = c.ckks_encrypt(enc, pk, hg.to_device(p2))

    def decode(dec, l):
        coeff = he.ntt_limbs(hg.to_host(dec).reshape(l, n), list(range(l)), inverse=True)
        return he.crt_centered(coeff, list(range(l)))[0]

    def share_noise(merged, ct, depth):
        l = Q - depth
        single = hg.to_host(c.ckks_decrypt(ct, s, depth)).reshape(l, n)
        q = np.array(primes[:l], dtype=np.uint64).reshape(l, 1)
        diff = (hg.to_host(merged).reshape(l, n) + q - single) % q
        return _centred_limbs(he.ntt_limbs(diff, list(range(l)), inverse=True), primes)

    # fresh ciphertext
    merged, _ = p.ckks_decrypt(ct1, 2 * Q * n)
    e = share_noise(merged, ct1, 0)
    print(f"{name} k={k}: max |sum of share errors| = {np.abs(e).max()} (bound {k * B})")
    assert np.abs(e).max() <= k * B
    x = decode(merged, Q)
    err = max(abs(int(a) - int(b) * scale) for a, b in zip(x, m1))
    print(f"{name} k={k}: fresh error {err} (margin {1 << 16})")
    assert err < 1 << 16
    # multiply + relinearize with the collective key
    out = torch.empty(3 * Q * n, dtype=torch.int64, device="cuda")
    c.ckks_multiply(ct1, 2 * Q * n, ct2, 2 * Q * n, out, 3 * Q * n, 0, 1)
    c.ckks_relinearize_inplace(out, 3 * Q * n, rk, 0, 1, c.workspace(hg.OP_CKKS_RELIN, 0, 1))
    ct3 = out[:2 * Q * n].contiguous()
    merged, _ = p.ckks_decrypt(ct3, 2 * Q * n)
    assert np.abs(share_noise(merged, ct3, 0)).max() <= k * B
    x = decode(merged, Q)
    err = max(abs(int(a) - int(b) * scale * scale) for a, b in zip(x, prod))
    print(f"{name} k={k}: error after multiply + relinearize {err} (margin {scale * scale // 2 ** 8})")
    assert err < scale * scale // 2 ** 8
    # rescale, then collective decryption one level down
    c.ckks_rescale_inplace(out, 3 * Q * n, 0, 1, c.workspace(hg.OP_CKKS_RESCALE, 0, 1))
    l = Q - 1
    ct4 = out[:2 * l * n].contiguous()
    merged, _ = p.ckks_decrypt(ct4, 2 * l * n, depth=1)
    assert np.abs(share_noise(merged, ct4, 1)).max() <= k * B
    x = decode(merged, l)
    q_last = primes[Q - 1]
    err = max(abs(int(a) * q_last - int(b) * scale * scale) for a, b in zip(x, prod))
    assert err < scale * scale // 2 ** 8
    # rotation with the collective Galois key
    rot = torch.empty(2 * Q * n, dtype=torch.int64, device="cuda")
    c.ckks_apply_galois(ct1, 2 * Q * n, rot, 2 * Q * n, gk, gal, 0, 1, c.workspace(hg.OP_CKKS_GALOIS, 0, 1))
    merged, _ = p.ckks_decrypt(rot, 2 * Q * n)
    x = decode(merged, Q)
    want = he.apply_galois_poly(np.array([int(v) * scale for v in m1], dtype=object), gal)
    err = max(abs(int(a) - int(b)) for a, b in zip(x, want))
    print(f"{name} k={k}: error after the rotation {err} (margin {scale // 2 ** 8})")
    assert err < scale // 2 ** 8


@pytest.mark.parametrize("k", PARTIES)
def test_bfv_collective_keys_and_decryption(hg, oracle, torch, k):
    """BFV: the merged plaintext EQUALS the message for a fresh ciphertext, after multiply + relinearize with the
    collective rk and after a rotation with the collective gk; the shares' sum differs from c1 * s by at most k * B."""
    c, o, primes, t = _bfv(hg, oracle)
    Q, Qp, n = c.Q_size, c.Q_prime_size, N
    he = RLWE(o, seed=0)
    p = Parties(hg, c, k)
    pk, rk = p.public_key(), p.relin_key()
    gal = hg.steps_to_galois_elt(1, n, 3)
    gk = p.galois_key(gal)
    s = p.sum_secret(primes)
    # the public key's noise, as for CKKS
    pkh = _limbs(pk, hg, Qp)
    noise = _sum_mod([pkh[0], _mul_mod(pkh[1], s, primes)], primes, Qp)[0]
    assert np.abs(_centred_limbs(he.ntt_limbs(noise, list(range(Qp)), inverse=True), primes)).max() <= k * B
    g = np.random.default_rng(8)
    m1, m2 = g.integers(0, t, n).astype(np.uint64), g.integers(0, t, n).astype(np.uint64)
    enc = hg.Rng(78)
    c1, c2 = c.bfv_encrypt(enc, pk, hg.to_device(m1)), c.bfv_encrypt(enc, pk, hg.to_device(m2))
    merged, shares = p.bfv_decrypt(c1, 2 * Q * n)
    assert np.array_equal(hg.to_host(merged), m1), "collective decryption of a fresh ciphertext"
    assert np.array_equal(hg.to_host(merged), hg.to_host(c.bfv_decrypt(c1, hg.to_device(s.reshape(-1)))))
    # sum of the shares - INTT(NTT(c1) * s) = the sum of the parties' errors (coefficient domain)
    ids = list(range(Q))
    c1_ntt = he.ntt_limbs(hg.to_host(c1).reshape(2, Q, n)[1], ids)
    c1s = he.ntt_limbs(_mul_mod(c1_ntt, s[:Q], primes), ids, inverse=True)
    q = np.array(primes[:Q], dtype=np.uint64).reshape(Q, 1)
    diff = (_sum_mod([hg.to_host(x) for x in shares], primes, Q)[0] + q - c1s) % q
    e = _centred_limbs(diff, primes)
    print(f"bfv k={k}: max |sum of share errors| = {np.abs(e).max()} (bound {k * B})")
    assert np.abs(e).max() <= k * B
    # multiply + relinearize with the collective key
    out = torch.empty(3 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_multiply(c1, 2 * Q * n, c2, 2 * Q * n, out, 3 * Q * n, 1, c.workspace(hg.OP_BFV_MULTIPLY, 0, 1))
    c.bfv_relinearize_inplace(out, 3 * Q * n, rk, 1, c.workspace(hg.OP_BFV_RELIN, 0, 1))
    merged, _ = p.bfv_decrypt(out[:2 * Q * n].contiguous(), 2 * Q * n)
    want = np.array([int(v) % t for v in negacyclic_mul(m1, m2)], dtype=np.uint64)
    assert np.array_equal(hg.to_host(merged), want), "collective decryption of relinearize(c1 * c2)"
    rot = torch.empty(2 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_apply_galois(c1, 2 * Q * n, rot, 2 * Q * n, gk, gal, 1, c.workspace(hg.OP_BFV_GALOIS, 0, 1))
    merged, _ = p.bfv_decrypt(rot, 2 * Q * n)
    want = np.array([int(v) % t for v in he.apply_galois_poly(m1.astype(object), gal)], dtype=np.uint64)
    assert np.array_equal(hg.to_host(merged), want), "collective decryption of rotate(c1)"


def test_common_randomness_and_determinism(hg, oracle, torch):
    c, o, primes = _ckks(hg, oracle, "method_I")
    Qp, d = c.Q_prime_size, c.switch_key_digits()
    gal = hg.steps_to_galois_elt(1, N, 5)

    def run(crs_seed, rng_seed):
        crs, rng = hg.Rng(crs_seed), hg.Rng(rng_seed)
        sk = c.generate_secret_key(rng)
        pk = c.mpc_public_key_share(crs, rng, sk)
        u, r1 = c.mpc_relin_key_share_round1(crs, rng, sk)
        gk = c.mpc_galois_key_share(crs, rng, sk, gal)
        r2 = c.mpc_relin_key_share_round2(rng, sk, u, r1)  # a one-party round-1 sum is the share itself
        ct = c.ckks_encrypt(hg.Rng(5), c.mpc_accumulate([pk], hg.MPC_PUBLIC_KEY), hg.to_device(np.zeros(c.Q_size * N, np.uint64)))
        h = c.mpc_ckks_decrypt_share(rng, ct, 2 * c.Q_size * N, sk)
        return [hg.to_host(x) for x in (pk, u, r1, gk, r2, h)]

    a, again, other_rng, other_crs = run(1, 10), run(1, 10), run(1, 11), run(2, 10)
    for x, y in zip(a, again):
        assert np.array_equal(x, y), "same seeds, same call order: the same bytes"
    pk_a, pk_r, pk_c = (x[0].reshape(2, Qp, N) for x in (a, other_rng, other_crs))
    assert np.array_equal(pk_a[1], pk_r[1]) and not np.array_equal(pk_a[1], pk_c[1]), "a follows the crs seed alone"
    assert not np.array_equal(pk_a[0], pk_r[0]), "the first part follows the party's own generator"
    gk_a, gk_r, gk_c = (x[3].reshape(d, 2, Qp, N) for x in (a, other_rng, other_crs))
    assert np.array_equal(gk_a[:, 1], gk_r[:, 1]) and not np.array_equal(gk_a[:, 1], gk_c[:, 1])
    assert not np.array_equal(gk_a[:, 0], gk_r[:, 0])
    assert not np.array_equal(a[2], other_rng[2]) and not np.array_equal(a[1], other_rng[1]), "round 1 and u are private"


def test_refusals_leave_the_context_usable(hg, oracle, torch):
    c, o, primes = _ckks(hg, oracle, "method_I")
    cb, _, _, _ = _bfv(hg, oracle)
    lib = hg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    crs, rng = hg.Rng(1), hg.Rng(2)
    sk = c.generate_secret_key(rng)
    gal = hg.steps_to_galois_elt(1, N, 5)

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value

    refused(lambda: c.mpc_public_key_share(rng, rng, sk))
    refused(lambda: c.mpc_relin_key_share_round1(crs, crs, sk))
    refused(lambda: c.mpc_galois_key_share(rng, rng, sk, gal))
    share = c.mpc_public_key_share(crs, rng, sk)
    refused(lambda: c.mpc_accumulate([], hg.MPC_PUBLIC_KEY))
    refused(lambda: c.mpc_accumulate([share, None], hg.MPC_PUBLIC_KEY))
    refused(lambda: c.mpc_accumulate([share], 7))
    pk = c.mpc_accumulate([share], hg.MPC_PUBLIC_KEY)
    ct = c.ckks_encrypt(hg.Rng(3), pk, hg.to_device(np.zeros(c.Q_size * N, np.uint64)))
    words = 2 * c.Q_size * N
    h = c.mpc_ckks_decrypt_share(rng, ct, words, sk)
    refused(lambda: c.mpc_ckks_decrypt_merge(ct, words, []))
    refused(lambda: c.mpc_ckks_decrypt_merge(ct, words, [None]))
    refused(lambda: c.mpc_ckks_decrypt_share(rng, ct, words, sk, depth=c.Q_size))
    refused(lambda: c.mpc_ckks_decrypt_merge(ct, words, [h], depth=-1))
    refused(lambda: c.mpc_relin_key_finish([], share))
    # a context of the other scheme
    refused(lambda: cb.mpc_ckks_decrypt_share(rng, ct, words, sk))
    refused(lambda: cb.mpc_ckks_decrypt_merge(ct, words, [h]))
    refused(lambda: c.mpc_bfv_decrypt_share(rng, ct, words, sk))
    refused(lambda: c.mpc_bfv_decrypt_merge(ct, words, [h]))
    # a null share buffer
    ws = c.workspace(hg.OP_MPC_KEY_SHARE, 0, 1)
    assert lib.hegpu_mpc_public_key_share(c._h, crs._h, rng._h, sk.data_ptr(), None, ws.data_ptr(), ws.numel() * 8, st) == hg.E_INVALID
    assert lib.hegpu_mpc_ckks_decrypt_share(c._h, rng._h, ct.data_ptr(), words, sk.data_ptr(), 0, None, 1, st) == hg.E_INVALID
    assert lib.hegpu_mpc_public_key_share(c._h, crs._h, rng._h, sk.data_ptr(), share.data_ptr(), ws.data_ptr(), 8, st) == hg.E_INVALID
    # and the next valid calls still work: one party's collective decryption is an ordinary decryption plus one error
    merged = c.mpc_ckks_decrypt_merge(ct, words, [h])
    single = c.ckks_decrypt(ct, sk)
    assert merged.shape == single.shape and not np.array_equal(hg.to_host(merged), hg.to_host(single))
    torch.cuda.synchronize()


@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_batched_collective_decryption(hg, oracle, torch, scheme, batch):
    """one call for the whole batch = one call per ciphertext on the same shares, byte for byte; and a batched share
    carries one independent error per ciphertext: for a batch of COPIES of one ciphertext (equal c1 * s_i) no two items
    of a share are equal."""
    k, pad = 3, 640
    if scheme == "ckks":
        c, o, primes = _ckks(hg, oracle, "method_I")
        l = c.Q_size
    else:
        c, o, primes, t = _bfv(hg, oracle)
        l = c.Q_size
    n, words = N, 2 * l * N
    stride = words + pad
    p = Parties(hg, c, k)
    pk = p.public_key()
    enc = hg.Rng(4)
    g = np.random.default_rng(6)
    cts = []
    for b in range(batch):
        if scheme == "ckks":
            plain = np.concatenate([g.integers(0, primes[j], n, dtype=np.uint64) for j in range(l)])
            cts.append(c.ckks_encrypt(enc, pk, hg.to_device(plain)))
        else:
            cts.append(c.bfv_encrypt(enc, pk, hg.to_device(g.integers(0, t, n).astype(np.uint64))))
    buf = torch.zeros(batch * stride, dtype=torch.int64, device="cuda")
    for b, ct in enumerate(cts):
        buf[b * stride:b * stride + words] = ct
    dec = p.ckks_decrypt if scheme == "ckks" else p.bfv_decrypt
    merged, shares = dec(buf, stride, batch=batch)
    out_words = l * n if scheme == "ckks" else n
    merged = hg.to_host(merged).reshape(batch, out_words)
    for b in range(batch):
        item = [x[b * l * n:(b + 1) * l * n].contiguous() for x in shares]
        if scheme == "ckks":
            alone = c.mpc_ckks_decrypt_merge(cts[b], words, item)
        else:
            alone = c.mpc_bfv_decrypt_merge(cts[b], words, item)
            assert np.array_equal(hg.to_host(alone), hg.to_host(c.bfv_decrypt(cts[b], hg.to_device(p.sum_secret(primes).reshape(-1)))))
        assert np.array_equal(merged[b], hg.to_host(alone)), (scheme, batch, b)
    # independent errors
    copies = cts[0].repeat(batch)
    fn = c.mpc_ckks_decrypt_share if scheme == "ckks" else c.mpc_bfv_decrypt_share
    h = hg.to_host(fn(p.rng[0], copies, words, p.sk[0], batch=batch)).reshape(batch, l * n)
    for i in range(batch):
        for j in range(i + 1, batch):
            assert not np.array_equal(h[i], h[j]), (scheme, batch, i, j)


def test_more_shares_than_one_launch_takes(hg, oracle, torch):
    """20 shares (the kernels take 16 pointers per launch): accumulate and both merges still give the modular sum"""
    k = 20
    c, o, primes = _ckks(hg, oracle, "method_I")
    Q, Qp = c.Q_size, c.Q_prime_size
    g = np.random.default_rng(1)
    shares = [np.stack([g.integers(0, primes[j], N, dtype=np.uint64) for j in range(Qp)] * 2) for _ in range(k)]
    out = _limbs(c.mpc_accumulate([hg.to_device(x.reshape(-1)) for x in shares], hg.MPC_PUBLIC_KEY), hg, Qp)
    want = shares[0][:Qp]
    for x in shares[1:]:
        want = (want + x[:Qp]) % np.array(primes, dtype=np.uint64).reshape(Qp, 1)
    assert np.array_equal(out[0], want) and np.array_equal(out[1], shares[0][Qp:])
    ct = np.stack([g.integers(0, primes[j], N, dtype=np.uint64) for j in range(Q)] * 2)
    hs = [np.stack([g.integers(0, primes[j], N, dtype=np.uint64) for j in range(Q)]) for _ in range(k)]
    got = hg.to_host(c.mpc_ckks_decrypt_merge(hg.to_device(ct.reshape(-1)), 2 * Q * N, [hg.to_device(x.reshape(-1)) for x in hs]))
    want = ct[:Q]
    for x in hs:
        want = (want + x) % np.array(primes[:Q], dtype=np.uint64).reshape(Q, 1)
    assert np.array_equal(got.reshape(Q, N), want)
    cb, ob, pb, t = _bfv(hg, oracle)
    Qb = cb.Q_size
    pr = Parties(hg, cb, k)
    m = g.integers(0, t, N).astype(np.uint64)
    cbt = cb.bfv_encrypt(hg.Rng(2), pr.public_key(), hg.to_device(m))
    merged, _ = pr.bfv_decrypt(cbt, 2 * Qb * N)
    assert np.array_equal(hg.to_host(merged), m)


def test_second_share_group_and_strides_that_differ(hg, oracle, torch):
    """17 shares (a second group of one), batch 3, ciphertexts 64 words further apart than they are long, CKKS at depth 1
    of a three-prime chain: the second group must read the first group's sum at the OUTPUT's item stride, not the
    ciphertext's, and the shares' item stride is neither of them.  The padding holds random words, so a read at the wrong
    stride changes the result.  The decrypt share is checked on its own: share - c1 * s is the transform of one error
    polynomial per item, every coefficient a rounded Gaussian clipped at 6 sigma (at most B)."""
    k, batch, depth, pad = 17, 3, 1, 64
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [50, 30, 30], [50], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    l = c.Q_size - depth
    words, g = 2 * l * N, np.random.default_rng(31)
    stride = words + pad
    q = np.array(primes[:l], dtype=np.uint64).reshape(1, l, 1)

    def padded(items):
        buf = g.integers(0, 1 << 62, (batch, stride), dtype=np.uint64)
        buf[:, :words] = items.reshape(batch, words)
        return hg.to_device(buf.reshape(-1))

    def residues(parts):
        return np.stack([g.integers(0, primes[j], (batch, parts, N), dtype=np.uint64) for j in range(l)], axis=2)

    # ---- CKKS merge: c0 + the modular sum of the shares, item by item
    ct = residues(2)  # [batch][2][l][N]
    hs = [residues(1).reshape(batch, l, N) for _ in range(k)]
    got = hg.to_host(c.mpc_ckks_decrypt_merge(padded(ct), stride, [hg.to_device(x.reshape(-1)) for x in hs], depth, batch))
    want = ct[:, 0]
    for x in hs:
        want = (want + x) % q
    assert np.array_equal(got.reshape(batch, l, N), want), "merge of 17 strided shares"
    # ---- CKKS decrypt share: share - c1 * s = NTT(e), |e| <= B
    rng = hg.Rng(311)
    sk = c.generate_secret_key(rng)
    s = hg.to_host(sk).reshape(c.Q_prime_size, N)[:l]
    share = hg.to_host(c.mpc_ckks_decrypt_share(rng, padded(ct), stride, sk, depth, batch)).reshape(batch, l, N)
    diff = np.stack([(share[b] + q[0] - _mul_mod(ct[b, 1], s, primes)) % q[0] for b in range(batch)])
    dev = hg.to_device(diff.reshape(-1))
    c.ntt(dev, dev, True, batch * l, l)
    e = hg.to_host(dev).reshape(batch, l, N)
    worst = max(int(np.abs(_centred_limbs(e[b], primes)).max()) for b in range(batch))
    print(f"decrypt share at depth 1, batch 3, padded stride: max |e| = {worst} (bound {B})")
    assert worst <= B
    # ---- BFV merge: 17 real shares of three padded ciphertexts open to the messages
    cb, _, _, t = _bfv(hg, oracle)
    words = 2 * cb.Q_size * N
    stride = words + pad
    p = Parties(hg, cb, k)
    pk, enc = p.public_key(), hg.Rng(312)
    msgs = g.integers(0, t, (batch, N)).astype(np.uint64)
    cts = np.stack([hg.to_host(cb.bfv_encrypt(enc, pk, hg.to_device(m))) for m in msgs])
    merged, _ = p.bfv_decrypt(padded(cts), stride, batch=batch)
    assert np.array_equal(hg.to_host(merged).reshape(batch, N), msgs), "BFV merge of 17 strided shares"
