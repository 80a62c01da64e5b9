"""Collective ciphertext refresh through the C ABI (hegpu_mpc_{ckks,bfv}_refresh_{share,merge}), k = 1, 2, 3, 5 parties.

What is exact is checked exactly, against Python integers and the oracle's transforms:
  * the coordinator (sum, INTT, centred lift, NTT, sum; BFV: sum, scale-and-round, D(.)) on arbitrary share arrays,
    including coefficients on both sides of the centring threshold and every LMAX instance of the lift;
  * the common polynomial `a`, recomputed from the DRBG (hegpu_drbg_block) in the documented draw order.
What carries fresh randomness is checked against bounds that follow from the samplers alone: every error is a rounded
Gaussian clipped at 6 sigma = 19.2, hence B = 20 per error; a CKKS mask coefficient is uniform in
[-2^(mask_bits-1), 2^(mask_bits-1)), a BFV mask coefficient uniform in [0, t).

  * share identity:  (h0_i - c1 s_i) + (h1_i + a s_i) = e0 + e1, at most 2B, equal in every limb;
  * end to end:      c0' + c1' s = m~ + sum_i (e0_i + e1_i) in every one of the Q limbs, at most 2kB off, where m~ is
                     the centred value of c0 + c1 s modulo the level's modulus -- provided
                     k 2^(mask_bits-1) + |m~| + 2kB < Q_level / 2, which every test asserts from the known message
                     before it calls the entry;
  * P(no mask coefficient of 4096 exceeds 2^(mask_bits-4) in magnitude) = (2^-3)^4096 = 2^-12288.
"""
import ctypes

import numpy as np
import pytest

from he_math import RLWE, negacyclic_mul
from test_gpu_mpc import B, CKKS_SETS, N, PARTIES, Parties, _centred_limbs, _mul_mod

pytestmark = pytest.mark.gpu

CRS = 4242
CHAINS = dict(CKKS_SETS, limbs_20=([60] + [50] * 19, [60]), limbs_40=([60] + [50] * 39, [60]))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_cache = {}


def _ckks(hg, oracle, name):
    if name not in _cache:
        log_q, log_p = CHAINS[name]
        c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
        c.upload()
        _cache[name] = (c, o, primes)
    return _cache[name]


def _bfv(hg, oracle):
    if "bfv" not in _cache:
        t = 1032193
        c = hg.Context.from_default(hg.BFV, N, 1, t)
        primes = [int(x) for x in c.table("modulus")]
        o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, t)
        c.upload()
        _cache["bfv"] = (c, o, primes, t)
    return _cache["bfv"]


# ---------------------------------------------------------------- Python-integer model
def _prod(primes):
    M = 1
    for q in primes:
        M *= q
    return M


def _compose_centred(rns, primes):
    """[l][N] residues -> N Python integers in [-(M-1)/2, (M-1)/2]"""
    M = _prod(primes)
    acc = np.zeros(rns.shape[1], dtype=object)
    for j, q in enumerate(primes):
        Mi = M // q
        acc = (acc + rns[j].astype(object) * (Mi * pow(Mi % q, -1, q))) % M
    return np.array([int(x) - M if int(x) > M // 2 else int(x) for x in acc], dtype=object), M


def _to_rns(poly, primes):
    return np.stack([np.array([int(v) % q for v in poly], dtype=np.uint64) for q in primes])


def _add(a, b, primes, sub=False):
    out = np.empty_like(a)
    for j, q in enumerate(primes):
        x, y = a[j].astype(object), b[j].astype(object)
        out[j] = np.array((x - y) % q if sub else (x + y) % q, dtype=np.uint64)
    return out


def _rand_rns(g, primes, rows=None):
    return np.stack([g.integers(0, q, N, dtype=np.uint64) for q in primes])


def _common_a(hg, seed, stream, item, primes):
    """item `item` of a call made when Rng(seed) stood at stream id `stream`: a[j][n] = the 128 bits of DRBG block
    (stream + item, j * N + n) reduced modulo q_j"""
    lib = hg._lib.load()
    key = (int(seed) & (2**64 - 1)).to_bytes(8, "little") + bytes(24)
    w = (ctypes.c_uint32 * 4)()
    Q = len(primes)
    out = np.empty((Q, N), dtype=np.uint64)
    for j, q in enumerate(primes):
        for n in range(N):
            assert lib.hegpu_drbg_block(key, stream + item, j * N + n, w) == 0
            out[j, n] = (w[0] | (w[1] << 32) | (w[2] << 64) | (w[3] << 96)) % q
    return out


def _special_values(M):
    """coefficients on both sides of the centring threshold (M + 1) / 2, as canonical residues mod M"""
    h = (M - 1) // 2
    return [0, 1, M - 1, h, h + 1, h - 1, h + 2, 2, M - 2, M // 2, M // 3, M - M // 3]


def _bfv_scaled(m, primes, c):
    """D(m) [Q][N]: Delta m + floor((m (Q mod t) + upper_threshold) / t) limb by limb (hegpu_bfv_encrypt)"""
    cd = [int(x) for x in c.table("coeff_div_plain_modulus")]
    r, th, t = int(c.table("Q_mod_t")[0]), int(c.table("upper_threshold")[0]), _cache["bfv"][3]
    m = np.array([int(v) for v in m], dtype=object)
    fix = (m * r + th) // t
    return np.stack([np.array((m * cd[j] + fix) % q, dtype=np.uint64) for j, q in enumerate(primes)])


# ---------------------------------------------------------------- the coordinator is exact
@pytest.mark.parametrize("name,depth,k", [("method_I", 0, 1), ("method_I", 3, 2), ("method_I", 2, 3), ("method_II", 1, 5),
                                          ("method_II", 2, 2), ("limbs_20", 0, 2), ("limbs_20", 8, 3),
                                          ("limbs_20", 15, 1), ("limbs_40", 0, 2), ("limbs_40", 39, 1)])
def test_ckks_coordinator_is_exact(hg, oracle, torch, name, depth, k):
    """arbitrary shares; c0 chosen so that t = c0 + sum h0 has prescribed coefficients (0, +-1, +-(Q_level - 1)/2 and
    their neighbours first, uniform values after them).  l = Q - depth covers l = 1, l = Q and the lift's instances for
    up to 8, 16, 32 and 64 words."""
    c, o, primes = _ckks(hg, oracle, name)
    Q = c.Q_size
    l = Q - depth
    lvl, full = primes[:l], primes[:Q]
    he = RLWE(o, seed=3)
    g = np.random.default_rng(100 * depth + k)
    M = _prod(lvl)
    T = _special_values(M)
    T = T + [int.from_bytes(g.bytes(8 * l + 8), "little") % M for _ in range(N - len(T))]
    t_ntt = he.ntt_limbs(_to_rns(T, lvl), list(range(l)))
    shares = [np.concatenate([_rand_rns(g, lvl), _rand_rns(g, full)]) for _ in range(k)]
    h0_sum = np.zeros((l, N), dtype=np.uint64)
    for s in shares:
        h0_sum = _add(h0_sum, s[:l], lvl)
    c0 = _add(t_ntt, h0_sum, lvl, sub=True)
    ct = np.concatenate([c0, _rand_rns(g, lvl)])  # c1 is not read by the coordinator
    crs = hg.Rng(CRS)
    out = c.mpc_ckks_refresh_merge(crs, hg.to_device(ct.reshape(-1)), 2 * l * N,
                                   [hg.to_device(s.reshape(-1)) for s in shares], depth)
    got = hg.to_host(out).reshape(2, Q, N)
    # the model: the same sum, the oracle's INTT, Python integers, the oracle's NTT
    coeff = he.ntt_limbs(_add(c0, h0_sum, lvl), list(range(l)), inverse=True)
    x, _ = _compose_centred(coeff, lvl)
    assert [int(v) % M for v in x] == T, "the test's own construction"
    assert min(x) == -(M - 1) // 2 and max(x) == (M - 1) // 2, "both ends of the centred range occur"
    want0 = he.ntt_limbs(_to_rns(x, full), list(range(Q)))
    for s in shares:
        want0 = _add(want0, s[l:], full)
    assert np.array_equal(got[0], want0), (name, depth, k)
    assert np.array_equal(got[1], _common_a(hg, CRS, 0, 0, full)), "c1' = the crs's first draw of Q limbs"


@pytest.mark.parametrize("k", [1, 3, 17])
def test_bfv_coordinator_is_exact(hg, oracle, torch, k):
    """arbitrary shares; c0 chosen so that c0 + sum h0 = D(m) + e with |e| <= 40, whose scale-and-round is m: the output
    must be (sum h1 + D(m), INTT(a)) bit for bit"""
    c, o, primes, t = _bfv(hg, oracle)
    Q = c.Q_size
    full = primes[:Q]
    he = RLWE(o, seed=3)
    g = np.random.default_rng(k)
    m = g.integers(0, t, N)
    m[:4] = [0, 1, t - 1, t // 2]
    target = _add(_bfv_scaled(m, full, c), _to_rns(g.integers(-40, 41, N), full), full)
    shares = [np.concatenate([_rand_rns(g, full), _rand_rns(g, full)]) for _ in range(k)]
    h0_sum, h1_sum = np.zeros((Q, N), dtype=np.uint64), np.zeros((Q, N), dtype=np.uint64)
    for s in shares:
        h0_sum, h1_sum = _add(h0_sum, s[:Q], full), _add(h1_sum, s[Q:], full)
    ct = np.concatenate([_add(target, h0_sum, full, sub=True), _rand_rns(g, full)])
    out = c.mpc_bfv_refresh_merge(hg.Rng(CRS), hg.to_device(ct.reshape(-1)), 2 * Q * N,
                                  [hg.to_device(s.reshape(-1)) for s in shares])
    got = hg.to_host(out).reshape(2, Q, N)
    assert np.array_equal(got[0], _add(h1_sum, _bfv_scaled(m, full, c), full)), k
    a = _common_a(hg, CRS, 0, 0, full)
    assert np.array_equal(got[1], he.ntt_limbs(a, list(range(Q)), inverse=True)), "c1' = INTT(a)"


# ---------------------------------------------------------------- shares are what they claim
def _fresh_ckks(hg, c, he, p, Q, scale, m, seed=77):
    plain = he.to_ntt([int(v) * scale for v in m], range(Q)).reshape(-1)
    return c.ckks_encrypt(hg.Rng(seed), p.public_key(), hg.to_device(plain))


def _drop(ct, Q, l):
    """mod-drop of a [2][Q][N] ciphertext to its first l limbs (the scale stays)"""
    return ct.reshape(2, Q, N)[:, :l].contiguous().reshape(-1)


@pytest.mark.parametrize("k", PARTIES)
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_ckks_shares_are_what_they_claim(hg, oracle, torch, name, k):
    c, o, primes = _ckks(hg, oracle, name)
    Q, depth = c.Q_size, 1
    l = Q - depth
    lvl, full = primes[:l], primes[:Q]
    he = RLWE(o, seed=1)
    p = Parties(hg, c, k, crs_seed=CRS)
    m = np.random.default_rng(5).integers(-8, 9, N)
    ct = _drop(_fresh_ckks(hg, c, he, p, Q, 1 << 30, m), Q, l)
    mask_bits = _prod(lvl).bit_length() - 10
    crs = [hg.Rng(CRS) for _ in range(k)]
    shares = [hg.to_host(c.mpc_ckks_refresh_share(crs[i], p.rng[i], ct, 2 * l * N, p.sk[i], depth, mask_bits))
              .reshape(l + Q, N) for i in range(k)]
    again = hg.to_host(c.mpc_ckks_refresh_share(hg.Rng(CRS), p.rng[0], ct, 2 * l * N, p.sk[0], depth, mask_bits))
    a = _common_a(hg, CRS, 0, 0, full)
    c1 = hg.to_host(ct).reshape(2, l, N)[1]
    masks = []
    for i in range(k):
        s_i = hg.to_host(p.sk[i]).reshape(-1, N)
        d0 = _add(shares[i][:l], _mul_mod(c1, s_i[:l], lvl), lvl, sub=True)
        d1 = _add(shares[i][l:], _mul_mod(a, s_i[:Q], full), full)
        x0, _ = _compose_centred(he.ntt_limbs(d0, list(range(l)), inverse=True), lvl)   # e0 - M_i
        x1, _ = _compose_centred(he.ntt_limbs(d1, list(range(Q)), inverse=True), full)  # e1 + M_i
        both = x0 + x1
        print(f"{name} k={k} party {i}: max |e0 + e1| = {max(abs(int(v)) for v in both)} (bound {2 * B}), "
              f"max |mask| = 2^{max(abs(int(v)) for v in x1).bit_length()} (mask_bits {mask_bits})")
        assert max(abs(int(v)) for v in both) <= 2 * B
        assert all(-(1 << (mask_bits - 1)) - B <= int(v) < (1 << (mask_bits - 1)) + B for v in x1), "the mask's range"
        assert max(abs(int(v)) for v in x1) > 1 << (mask_bits - 4), "the mask fills its range"
        masks.append(x1)
    for i in range(1, k):
        assert not np.array_equal(masks[0], masks[i]), "two parties, two masks"
    assert not np.array_equal(again.reshape(l + Q, N), shares[0]), "two calls, two masks"


@pytest.mark.parametrize("k", PARTIES)
def test_bfv_shares_are_what_they_claim(hg, oracle, torch, k):
    c, o, primes, t = _bfv(hg, oracle)
    Q = c.Q_size
    full = primes[:Q]
    he = RLWE(o, seed=0)
    p = Parties(hg, c, k, crs_seed=CRS)
    m = np.random.default_rng(8).integers(0, t, N).astype(np.uint64)
    ct = c.bfv_encrypt(hg.Rng(78), p.public_key(), hg.to_device(m))
    a = _common_a(hg, CRS, 0, 0, full)
    ids = list(range(Q))
    c1_ntt = he.ntt_limbs(hg.to_host(ct).reshape(2, Q, N)[1], ids)
    Qv = _prod(full)
    masks = []
    for i in range(k):
        sh = hg.to_host(c.mpc_bfv_refresh_share(hg.Rng(CRS), p.rng[i], ct, 2 * Q * N, p.sk[i])).reshape(2, Q, N)
        s_i = hg.to_host(p.sk[i]).reshape(-1, N)[:Q]
        d0 = _add(sh[0], he.ntt_limbs(_mul_mod(c1_ntt, s_i, full), ids, inverse=True), full, sub=True)  # e0 - D(M)
        d1 = _add(sh[1], he.ntt_limbs(_mul_mod(a, s_i, full), ids, inverse=True), full)                # e1 + D(M)
        e = _centred_limbs(_add(d0, d1, full), full)
        print(f"bfv k={k} party {i}: max |e0 + e1| = {np.abs(e).max()} (bound {2 * B})")
        assert np.abs(e).max() <= 2 * B
        x1, _ = _compose_centred(d1, full)
        M_i = np.array([((int(v) % Qv) * t + Qv // 2) // Qv % t for v in x1], dtype=np.int64)  # round(t / Q * x)
        assert M_i.min() >= 0 and M_i.max() < t and M_i.max() > t - t // 8 and M_i.min() < t // 8
        back = _centred_limbs(_add(d1, _bfv_scaled(M_i, full, c), full, sub=True), full)        # = e1
        assert np.abs(back).max() <= B
        masks.append(M_i)
    for i in range(1, k):
        assert not np.array_equal(masks[0], masks[i])


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("k", PARTIES)
@pytest.mark.parametrize("deepest", [False, True], ids=["depth2", "deepest"])
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_ckks_refresh_end_to_end(hg, oracle, torch, name, deepest, k):
    """refresh at depth 2 (method_II: its deepest level) and at the deepest level, mask_bits = bits(Q_level) - 10; then
    multiply + relinearize + rescale with the collective key on the refreshed ciphertext -- impossible on an input at
    the deepest level, which has no modulus left to rescale by.  Margins as tests/test_gpu_mpc.py: 2^16 for a fresh
    ciphertext (the refresh adds at most 2kB <= 200), scale^2 / 2^8 after the multiplication."""
    c, o, primes = _ckks(hg, oracle, name)
    Q = c.Q_size
    depth = Q - 1 if deepest else min(2, Q - 1)
    l = Q - depth
    lvl, full = primes[:l], primes[:Q]
    he = RLWE(o, seed=1)
    p = Parties(hg, c, k, crs_seed=CRS)
    rk = p.relin_key()
    s = p.sum_secret(primes)
    scale = 1 << 30
    g = np.random.default_rng(12)
    m1, m2 = g.integers(-8, 9, N), g.integers(-8, 9, N)
    ct1 = _fresh_ckks(hg, c, he, p, Q, scale, m1, 77)
    ct2 = _fresh_ckks(hg, c, he, p, Q, scale, m2, 79)
    ct_in = _drop(ct1, Q, l)
    Ql = _prod(lvl)
    mask_bits = Ql.bit_length() - 10
    # the protocol's condition, from the known message: |m~| <= 8 scale + the fresh ciphertext's noise (< 2^16)
    assert k * (1 << (mask_bits - 1)) + 8 * scale + (1 << 16) + 2 * k * B < Ql // 2
    host = hg.to_host(ct_in).reshape(2, l, N)
    m_tilde, _ = _compose_centred(he.ntt_limbs(_add(host[0], _mul_mod(host[1], s[:l], lvl), lvl), list(range(l)),
                                               inverse=True), lvl)
    assert max(abs(int(a) - int(b) * scale) for a, b in zip(m_tilde, m1)) < 1 << 16
    # parties and coordinator: generators advanced alike (Parties used p.crs for the keys; fresh ones here)
    shares = [c.mpc_ckks_refresh_share(hg.Rng(CRS), p.rng[i], ct_in, 2 * l * N, p.sk[i], depth, mask_bits)
              for i in range(k)]
    out = c.mpc_ckks_refresh_merge(hg.Rng(CRS), ct_in, 2 * l * N, shares, depth)
    oh = hg.to_host(out).reshape(2, Q, N)
    dec = _add(oh[0], _mul_mod(oh[1], s[:Q], full), full)
    diff = _add(he.ntt_limbs(dec, list(range(Q)), inverse=True), _to_rns(m_tilde, full), full, sub=True)
    e = _centred_limbs(diff, full)
    print(f"{name} depth={depth} k={k}: max |c0' + c1' s - lift(m~)| = {np.abs(e).max()} (bound {2 * k * B})")
    assert np.abs(e).max() <= 2 * k * B
    x, _ = _compose_centred(he.ntt_limbs(dec, list(range(Q)), inverse=True), full)
    err = max(abs(int(a) - int(b) * scale) for a, b in zip(x, m1))
    print(f"{name} depth={depth} k={k}: error of the refreshed ciphertext {err} (margin {1 << 16})")
    assert err < 1 << 16
    # the refreshed ciphertext computes again
    prod3 = torch.empty(3 * Q * N, dtype=torch.int64, device="cuda")
    c.ckks_multiply(out, 2 * Q * N, ct2, 2 * Q * N, prod3, 3 * Q * N, 0, 1)
    c.ckks_relinearize_inplace(prod3, 3 * Q * N, rk, 0, 1, c.workspace(hg.OP_CKKS_RELIN, 0, 1))
    c.ckks_rescale_inplace(prod3, 3 * Q * N, 0, 1, c.workspace(hg.OP_CKKS_RESCALE, 0, 1))
    l1 = Q - 1
    ct4 = prod3[:2 * l1 * N].contiguous()
    merged, _ = p.ckks_decrypt(ct4, 2 * l1 * N, depth=1)
    coeff = he.ntt_limbs(hg.to_host(merged).reshape(l1, N), list(range(l1)), inverse=True)
    x, _ = _compose_centred(coeff, primes[:l1])
    want = negacyclic_mul(m1, m2)
    err = max(abs(int(a) * primes[Q - 1] - int(b) * scale * scale) for a, b in zip(x, want))
    print(f"{name} depth={depth} k={k}: error after multiply + relinearize + rescale {err} (margin {scale * scale // 2 ** 8})")
    assert err < scale * scale // 2 ** 8


def _bfv_noise(hg, c, ct, s_dev, primes, torch):
    """max |t (c0 + c1 s) mod Q| (centred) through hegpu_bfv_noise_rns"""
    Q = c.Q_size
    out = torch.empty(Q * N, dtype=torch.int64, device="cuda")
    rc = hg._lib.load().hegpu_bfv_noise_rns(c._h, ct.data_ptr(), s_dev.data_ptr(), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    x, _ = _compose_centred(hg.to_host(out).reshape(Q, N), primes[:Q])
    return max(abs(int(v)) for v in x)


@pytest.mark.parametrize("k", PARTIES)
def test_bfv_refresh_end_to_end(hg, oracle, torch, k):
    """The refreshed ciphertext is (sum_i (h1_i) + D(m'), INTT(a)) with c0' + c1' s = sum_i e1_i + sum_i D(M_i) + D(m')
    and m' + sum_i M_i = m + z t, |z| <= k.  With r = Q mod t, t D(u) = t Delta u + t round(u r / t) = (Q - r) u + u r +
    d_u = Q u + d_u, |d_u| <= t / 2 + 1 (the rounding of the fix), so modulo Q
        t (c0' + c1' s) = t sum_i e1_i + sum of k + 1 terms d_u,   at most  t k B + (k + 1) (t / 2 + 1)
    whatever noise the input carried.  hegpu_bfv_noise_rns measures exactly this quantity; the input here is a product
    of two fresh ciphertexts, whose noise is far above that."""
    c, o, primes, t = _bfv(hg, oracle)
    Q = c.Q_size
    full = primes[:Q]
    p = Parties(hg, c, k, crs_seed=CRS)
    pk, rk = p.public_key(), p.relin_key()
    s_dev = hg.to_device(p.sum_secret(primes).reshape(-1))
    g = np.random.default_rng(8)
    m1, m2, m3 = (g.integers(0, t, N).astype(np.uint64) for _ in range(3))
    enc = hg.Rng(78)
    c1, c2, c3 = (c.bfv_encrypt(enc, pk, hg.to_device(m)) for m in (m1, m2, m3))

    def mul(x, y):
        out = torch.empty(3 * Q * N, dtype=torch.int64, device="cuda")
        c.bfv_multiply(x, 2 * Q * N, y, 2 * Q * N, out, 3 * Q * N, 1, c.workspace(hg.OP_BFV_MULTIPLY, 0, 1))
        c.bfv_relinearize_inplace(out, 3 * Q * N, rk, 1, c.workspace(hg.OP_BFV_RELIN, 0, 1))
        return out[:2 * Q * N].contiguous()

    ct_in = mul(c1, c2)
    m12 = np.array([int(v) % t for v in negacyclic_mul(m1, m2)], dtype=np.uint64)
    shares = [c.mpc_bfv_refresh_share(hg.Rng(CRS), p.rng[i], ct_in, 2 * Q * N, p.sk[i]) for i in range(k)]
    out = c.mpc_bfv_refresh_merge(hg.Rng(CRS), ct_in, 2 * Q * N, shares)
    assert np.array_equal(hg.to_host(c.bfv_decrypt(out, s_dev)), m12), "the refreshed ciphertext holds the same plaintext"
    noise_in, noise_out = _bfv_noise(hg, c, ct_in, s_dev, primes, torch), _bfv_noise(hg, c, out, s_dev, primes, torch)
    bound = t * k * B + (k + 1) * (t // 2 + 1)
    print(f"bfv k={k}: t * noise before 2^{noise_in.bit_length()}, after {noise_out} (bound {bound})")
    assert noise_out <= bound and noise_out < noise_in
    ct5 = mul(out, c3)
    want = np.array([int(v) % t for v in negacyclic_mul(m12, m3)], dtype=np.uint64)
    assert np.array_equal(hg.to_host(c.bfv_decrypt(ct5, s_dev)), want), "single-key decryption under s"
    merged, _ = p.bfv_decrypt(ct5, 2 * Q * N)
    assert np.array_equal(hg.to_host(merged), want), "collective decryption"


# ---------------------------------------------------------------- batches and edges
@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_batched_refresh_equals_item_by_item(hg, oracle, torch, scheme, batch):
    """padded strides in and out.  Every item takes stream ids of its own, so `batch` successive calls of one item, made
    with generators that start where the batched call's started, must reproduce the batched shares and the batched
    result item by item, byte for byte; and two runs from the same seeds are bit-equal."""
    k, pad = 3, 640
    if scheme == "ckks":
        c, o, primes = _ckks(hg, oracle, "method_I")
        depth = 1
    else:
        c, o, primes, t = _bfv(hg, oracle)
        depth = 0
    Q = c.Q_size
    l = Q - depth
    full = primes[:Q]
    he = RLWE(o, seed=2)
    in_words, out_words = 2 * l * N, 2 * Q * N
    share_words = (l + Q) * N
    cs, so = in_words + pad, out_words + 2 * pad
    p = Parties(hg, c, k, crs_seed=CRS)
    g = np.random.default_rng(6)
    buf = torch.zeros(batch * cs, dtype=torch.int64, device="cuda")
    items = []
    for b in range(batch):
        ct = np.concatenate([_rand_rns(g, primes[:l]), _rand_rns(g, primes[:l])]).reshape(-1)
        items.append(hg.to_device(ct))
        buf[b * cs:b * cs + in_words] = items[-1]
    mask_bits = 40

    def share(i, crs, rng, ct, stride, nb):
        if scheme == "ckks":
            return c.mpc_ckks_refresh_share(crs, rng, ct, stride, p.sk[i], depth, mask_bits, batch=nb)
        return c.mpc_bfv_refresh_share(crs, rng, ct, stride, p.sk[i], batch=nb)

    def merge(crs, ct, stride, shares, nb, out=None, out_stride=None):
        if scheme == "ckks":
            return c.mpc_ckks_refresh_merge(crs, ct, stride, shares, depth, batch=nb, out=out, out_stride=out_stride)
        return c.mpc_bfv_refresh_merge(crs, ct, stride, shares, batch=nb, out=out, out_stride=out_stride)

    def run():
        shares = [share(i, hg.Rng(CRS), hg.Rng(500 + i), buf, cs, batch) for i in range(k)]
        out = torch.full((batch * so,), -1, dtype=torch.int64, device="cuda")
        merge(hg.Rng(CRS), buf, cs, shares, batch, out, so)
        return shares, out

    shares, out = run()
    shares2, out2 = run()
    assert torch.equal(out, out2) and all(torch.equal(x, y) for x, y in zip(shares, shares2)), "same seeds, same bytes"
    oh = hg.to_host(out).reshape(batch, so)
    assert np.all(oh[:, out_words:] == np.uint64(2**64 - 1)), "the padding between the items is not written"
    # item by item, the generators advancing from call to call
    crs_p, rng_p, crs_c = [hg.Rng(CRS) for _ in range(k)], [hg.Rng(500 + i) for i in range(k)], hg.Rng(CRS)
    for b in range(batch):
        alone = [share(i, crs_p[i], rng_p[i], items[b], in_words, 1) for i in range(k)]
        for i in range(k):
            assert torch.equal(alone[i], shares[i][b * share_words:(b + 1) * share_words]), (scheme, batch, b, i)
        one = merge(crs_c, items[b], in_words, alone, 1)
        assert np.array_equal(hg.to_host(one), oh[b, :out_words]), (scheme, batch, b)
    # item b's a is the b-th draw of Q limbs
    for b in sorted({0, batch - 1}):
        a_b = oh[b, Q * N:out_words].reshape(Q, N)
        if scheme == "bfv":
            a_b = he.ntt_limbs(a_b, list(range(Q)))  # c1' = INTT(a)
        assert np.array_equal(a_b, _common_a(hg, CRS, 0, b, full)), (scheme, batch, b)
    sh = hg.to_host(shares[0]).reshape(batch, share_words)
    for i in range(batch):
        for j in range(i + 1, min(batch, i + 3)):
            assert not np.array_equal(sh[i], sh[j]), "one mask per item"


@pytest.mark.parametrize("k", [17, 33])
def test_more_refresh_shares_than_one_launch_takes(hg, oracle, torch, k):
    """the k-way sums take 16 pointers per launch: part 0 of the CKKS result is linear in the h1 halves, so with the
    shares' h0 halves all zero except the first share's, the result = the one-share result + the sum of the other h1"""
    c, o, primes = _ckks(hg, oracle, "method_I")
    Q, depth = c.Q_size, 1
    l = Q - depth
    lvl, full = primes[:l], primes[:Q]
    g = np.random.default_rng(k)
    ct = np.concatenate([_rand_rns(g, lvl), _rand_rns(g, lvl)])
    shares = [np.concatenate([_rand_rns(g, lvl), _rand_rns(g, full)]) for _ in range(k)]
    # fold the h0 halves of shares 1.. into share 0 for the reference run: the same t
    folded = shares[0].copy()
    for s in shares[1:]:
        folded[:l] = _add(folded[:l], s[:l], lvl)
    dev = lambda x: hg.to_device(x.reshape(-1))
    one = hg.to_host(c.mpc_ckks_refresh_merge(hg.Rng(CRS), dev(ct), 2 * l * N, [dev(folded)], depth)).reshape(2, Q, N)
    got = hg.to_host(c.mpc_ckks_refresh_merge(hg.Rng(CRS), dev(ct), 2 * l * N, [dev(s) for s in shares], depth)).reshape(2, Q, N)
    want0 = one[0]
    for s in shares[1:]:
        want0 = _add(want0, s[l:], full)
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], one[1])
    # BFV: the real protocol with k parties
    cb, ob, pb, t = _bfv(hg, oracle)
    Qb = cb.Q_size
    pr = Parties(hg, cb, k, crs_seed=CRS)
    m = g.integers(0, t, N).astype(np.uint64)
    cbt = cb.bfv_encrypt(hg.Rng(2), pr.public_key(), hg.to_device(m))
    sh = [cb.mpc_bfv_refresh_share(hg.Rng(CRS), pr.rng[i], cbt, 2 * Qb * N, pr.sk[i]) for i in range(k)]
    out = cb.mpc_bfv_refresh_merge(hg.Rng(CRS), cbt, 2 * Qb * N, sh)
    s_dev = hg.to_device(pr.sum_secret(pb).reshape(-1))
    assert np.array_equal(hg.to_host(cb.bfv_decrypt(out, s_dev)), m)


def test_refresh_refusals_and_empty_batch(hg, oracle, torch):
    c, o, primes = _ckks(hg, oracle, "method_I")
    cb, _, _, _ = _bfv(hg, oracle)
    lib = hg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    Q = c.Q_size
    words = 2 * Q * N
    crs, rng = hg.Rng(1), hg.Rng(2)
    sk = c.generate_secret_key(rng)
    skb = cb.generate_secret_key(rng)
    ct = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctb = torch.zeros(2 * cb.Q_size * N, dtype=torch.int64, device="cuda")
    bits = _prod(primes[:Q]).bit_length()

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value

    good = c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, 0, 40)
    goodb = cb.mpc_bfv_refresh_share(crs, rng, ctb, ctb.numel(), skb)
    refused(lambda: c.mpc_ckks_refresh_share(rng, rng, ct, words, sk, 0, 40))
    refused(lambda: cb.mpc_bfv_refresh_share(rng, rng, ctb, ctb.numel(), skb))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, None, words, sk, 0, 40))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, words, None, 0, 40))
    refused(lambda: cb.mpc_bfv_refresh_share(crs, rng, ctb, ctb.numel(), None))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, Q, 40))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, -1, 40))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, 0, 0))
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, 0, 127))
    # the mask rule: 2^mask_bits >= Q_level / 2 is refused, one bit less is accepted (depth Q - 1: the 50-bit level)
    b1 = primes[0].bit_length()
    l1 = 2 * N
    refused(lambda: c.mpc_ckks_refresh_share(crs, rng, ct, l1, sk, Q - 1, b1 - 1))
    c.mpc_ckks_refresh_share(crs, rng, ct, l1, sk, Q - 1, b1 - 2)
    assert bits > 127  # at depth 0 the cap of 126 bits is what binds
    c.mpc_ckks_refresh_share(crs, rng, ct, words, sk, 0, 126)
    # wrong scheme
    refused(lambda: cb.mpc_ckks_refresh_share(crs, rng, ct, words, sk, 0, 40))
    refused(lambda: c.mpc_bfv_refresh_share(crs, rng, ct, words, sk))
    refused(lambda: cb.mpc_ckks_refresh_merge(crs, ct, words, [good], 0))
    refused(lambda: c.mpc_bfv_refresh_merge(crs, ct, words, [good]))
    # shares
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [], 0))
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [good, None], 0))
    refused(lambda: cb.mpc_bfv_refresh_merge(crs, ctb, ctb.numel(), []))
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [good], Q))
    # out overlapping the input or a share
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [good], 0, out=ct))
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [good], 0, out=good))
    refused(lambda: c.mpc_ckks_refresh_merge(crs, ct, words, [good], 0, out=good[N:]))
    refused(lambda: cb.mpc_bfv_refresh_merge(crs, ctb, ctb.numel(), [goodb], out=ctb))
    refused(lambda: cb.mpc_bfv_refresh_merge(crs, ctb, ctb.numel(), [goodb], out=goodb))
    # null generators, a workspace that is too small
    ws = c.workspace(hg.OP_MPC_REFRESH_MERGE, 0, 1)
    out = torch.empty(words, dtype=torch.int64, device="cuda")
    arr = (ctypes.c_void_p * 1)(good.data_ptr())
    assert c.workspace_bytes(hg.OP_MPC_REFRESH_MERGE, 0, 1) == Q * N * 8
    assert c.workspace_bytes(hg.OP_MPC_REFRESH_MERGE, 1, 3) == 3 * (Q - 1) * N * 8
    assert cb.workspace_bytes(hg.OP_MPC_REFRESH_MERGE, 0, 2) == 2 * (cb.Q_size + 1) * N * 8
    assert c.workspace_bytes(hg.OP_MPC_REFRESH_SHARE, 0, 5) == 0
    assert lib.hegpu_mpc_ckks_refresh_merge(c._h, None, ct.data_ptr(), words, arr, 1, 0, out.data_ptr(), words, 1,
                                            ws.data_ptr(), ws.numel() * 8, st) == hg.E_INVALID
    assert lib.hegpu_mpc_ckks_refresh_merge(c._h, crs._h, ct.data_ptr(), words, arr, 1, 0, out.data_ptr(), words, 1,
                                            ws.data_ptr(), 8, st) == hg.E_INVALID
    assert lib.hegpu_mpc_ckks_refresh_merge(c._h, crs._h, ct.data_ptr(), words, arr, 1, 0, None, words, 1,
                                            ws.data_ptr(), ws.numel() * 8, st) == hg.E_INVALID
    assert lib.hegpu_mpc_ckks_refresh_share(c._h, None, rng._h, ct.data_ptr(), words, sk.data_ptr(), 0, 40,
                                            good.data_ptr(), 1, None, 0, st) == hg.E_INVALID
    assert lib.hegpu_mpc_ckks_refresh_share(c._h, crs._h, rng._h, ct.data_ptr(), words, sk.data_ptr(), 0, 40, None, 1,
                                            None, 0, st) == hg.E_INVALID
    # batch 0: a no-op that returns 0 and touches nothing, null pointers included
    before = good.clone()
    assert lib.hegpu_mpc_ckks_refresh_share(c._h, crs._h, rng._h, None, 0, None, 0, 40, good.data_ptr(), 0, None, 0, st) == 0
    assert lib.hegpu_mpc_ckks_refresh_merge(c._h, crs._h, None, 0, None, 0, 0, None, 0, 0, None, 0, st) == 0
    assert lib.hegpu_mpc_bfv_refresh_share(cb._h, crs._h, rng._h, None, 0, None, None, 0, None, 0, st) == 0
    assert lib.hegpu_mpc_bfv_refresh_merge(cb._h, crs._h, None, 0, None, 0, None, 0, 0, None, 0, st) == 0
    assert torch.equal(before, good)
    assert lib.hegpu_mpc_ckks_refresh_share(c._h, crs._h, rng._h, ct.data_ptr(), words, sk.data_ptr(), 0, 40,
                                            good.data_ptr(), -1, None, 0, st) == hg.E_INVALID
    # and the context still works
    c.mpc_ckks_refresh_merge(crs, ct, words, [good], 0)
    torch.cuda.synchronize()
