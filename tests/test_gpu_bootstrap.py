"""The assembled CKKS refresh (hegpu_ckks_bootstrap over heongpu_amd.api.bootstrap_plan), N = 4096.

Two 18-limb chains, low index first, three pieces each way, degree 30, r = 3, K = 12, ratio 256, scale 2^40:
  A  {50, 40, 40 x 3, 40, 50 x 8, 50, 50 x 3} | {60}      FP64 paths       k1 = 4
  B  {60, 40, 40 x 3, 40, 60 x 8, 56, 56 x 3} | {60}      integer paths    k1 = 4096
  method II: chain A with the special primes {60, 60}.
From the top: 3 limbs CoeffToSlot, 1 the split drops, 8 EvalMod, 1 the merge drops, 3 SlotToCoeff; two limbs are left.

  1. the entry against the chain of single entries (hegpu_ckks_constant_op, _apply_galois with the element 1,
     _mod_raise, _apply_galois, _coeff_to_slot, _poly_eval at batch 2 B, _slot_to_coeff) on synthetic keys, diagonals and
     inputs: exact; the padding between items and a guard word behind the workspace are untouched, inputs are not written;
  2. encrypted accuracy with real keys: (a) a secret of Hamming weight 32, no switch keys, (b) a dense secret, an ephemeral
     sparse one of weight 32 and both switch keys.  First the precondition: every overflow I of the raise is below K
     (decrypted on the host from the raised ciphertext; with weight 32 its deviation is about 1.7, K = 12 is seven sigma,
     no coefficient is excused).  Then max |decode(decrypt(out)) - f(a)| < 1e-4 over all N coefficients, f(a) =
     (rho / 2 pi) sin(2 pi a / rho), rho = q_0 / (k1 scale): the criterion of this repository's semantic tests.  Noise is
     expected near 1e-6 (key-switch noise 2^12 against a payload of 2^42, the forward factors amplify it); anything
     structural -- a wrong half, bit reversal, sign, an I outside K, a label off by a prime -- gives an error of order |a|;
  3. EvalMod alone under encryption: u = (I + eps) / K for every |I| <= 11, |eps| <= 2^-9, against the numpy model of
     tests/test_eval_mod_plan.py (copied), |y_r - model| rho < 1e-4;
  4. refusals launch nothing.
The measured figures are printed and recorded in DESIGN.md 4.5f."""
import math

import numpy as np
import pytest

from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
SLOTS = N // 2
SENT = 0x5555555555555555
DELTA = 2.0 ** 40
K, DEGREE, R = 12, 30, 3
CHAINS = {
    "A": ([50, 40, 40, 40, 40, 40] + [50] * 8 + [50] + [50] * 3, [60]),
    "B": ([60, 40, 40, 40, 40, 40] + [60] * 8 + [56] + [56] * 3, [60]),
    "A_method_II": ([50, 40, 40, 40, 40, 40] + [50] * 8 + [50] + [50] * 3, [60, 60]),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_context(hg, name):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *CHAINS[name], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    return c, primes


# ---------------------------------------------------------------- 1. the entry against the chain of single entries
_synthetic = {}


def synthetic(hg, name, ratio):
    """context, plan, synthetic factors and keys of one chain (kept for the module)"""
    if (name, ratio) in _synthetic:
        return _synthetic[(name, ratio)]
    if name not in _synthetic:
        c, primes = make_context(hg, name)
        key = lambda seed: hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, seed))  # noqa: E731
        _synthetic[name] = (c, primes, [key(11), key(12), key(13)], {k: key(20 + i) for i, k in enumerate(("conj", "relin", "d2s", "s2d"))})
    c, primes, pool, keys = _synthetic[name]
    plan = hg.bootstrap_plan(primes[:c.Q_size], DELTA, c.Q_size - 1, K=K, message_ratio=ratio)
    seed = [0]

    def encode(values, scale, limbs):  # residues in place of an encoded diagonal
        seed[0] += 1
        return hg.to_device(synth_ct(primes, range(limbs), 1, N, 5000 + seed[0]))
    cts, stc, elts = c.bootstrap_factors(plan, lambda e: pool[e % 3], encode)
    _synthetic[(name, ratio)] = (c, primes, plan, cts, stc, keys)
    return _synthetic[(name, ratio)]


def chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, cs, batch, with_keys):
    """the refresh entry by entry, every intermediate in a buffer of its own; returns the result, items out_words apart"""
    Q = c.Q_size
    new = lambda words: torch.full((words,), SENT, dtype=torch.int64, device="cuda")  # noqa: E731
    gal_ws = lambda depth: c.workspace(hg.OP_CKKS_GALOIS, depth, batch)  # noqa: E731
    cur, stride = ct, cs
    if plan.k1 != 1:
        cur = torch.cat([c.ckks_constant_op(2, ct[b * cs:b * cs + 2 * N].clone(), float(plan.k1), 1) for b in range(batch)])
        stride = 2 * N
    if with_keys:
        sparse = new(batch * 2 * N)
        c.ckks_apply_galois(cur, stride, sparse, 2 * N, keys["d2s"], 1, Q - 1, batch, gal_ws(Q - 1))
        cur, stride = sparse, 2 * N
    raise_depth = Q - 1 - plan.cts_level
    rs = 2 * (plan.cts_level + 1) * N
    raised = new(batch * rs)
    c.ckks_mod_raise(cur, stride, raised, rs, raise_depth, batch, c.workspace(hg.OP_CKKS_MOD_RAISE, raise_depth, batch))
    if with_keys:
        dense = new(batch * rs)
        c.ckks_apply_galois(raised, rs, dense, rs, keys["s2d"], 1, raise_depth, batch, gal_ws(raise_depth))
        raised = dense
    hs = 2 * (plan.eval_level + 1) * N
    halves = new(2 * batch * hs)
    ws = torch.empty(c.encoding_transform_workspace_bytes(cts, raise_depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_coeff_to_slot(raised, rs, halves[:batch * hs], halves[batch * hs:], hs, cts, keys["conj"], raise_depth, batch, ws)
    em = plan.eval_mod
    es = 2 * em.out_limbs * N
    sines = new(2 * batch * es)
    depth = Q - 1 - plan.eval_level
    ws = torch.empty(c.poly_eval_workspace_bytes(em, depth, 2 * batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_poly_eval(halves, hs, sines, es, em, keys["relin"], depth, 2 * batch, ws)
    room = 2 * (plan.out_level + 2) * N
    out = new(batch * room)
    depth = Q - 1 - plan.stc_level
    ws = torch.empty(c.encoding_transform_workspace_bytes(stc, depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_slot_to_coeff(sines[:batch * es], es, sines[batch * es:], es, out, room, stc, depth, batch, ws)
    return out, room, raised, rs


CASES = [(name, 256.0, batch, with_keys) for name in CHAINS for batch in (1, 2) for with_keys in (False, True)]
CASES += [("A", 1000.0, 1, False), ("A", 1000.0, 2, True)]  # k1 = 1: no multiplication at all


@pytest.mark.parametrize("name,ratio,batch,with_keys", CASES)
def test_entry_equals_the_chain_of_single_entries(hg, torch, name, ratio, batch, with_keys):
    c, primes, plan, cts, stc, keys = synthetic(hg, name, ratio)
    assert plan.k1 == {("A", 256.0): 4, ("B", 256.0): 4096, ("A_method_II", 256.0): 4, ("A", 1000.0): 1}[(name, ratio)]
    assert (plan.cts_level, plan.eval_level, plan.stc_level, plan.out_level) == (17, 13, 5, 1)
    cs = 2 * N + N  # N words of padding between the items
    cbuf = np.full(batch * cs, SENT, dtype=np.uint64)
    for b in range(batch):  # distinct items
        cbuf[b * cs:b * cs + 2 * N] = synth_ct(primes, [0], 2, N, 900 + b)
    ct = hg.to_device(cbuf)
    ow, room = 2 * (plan.out_level + 1) * N, 2 * (plan.out_level + 2) * N
    so = room + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    need = c.bootstrap_workspace_bytes(plan, cts, stc, with_keys, batch)
    assert need > c.workspace_bytes(hg.OP_CKKS_BOOTSTRAP, 0, batch) == 6 * N * 8 * batch
    ws = torch.full((need // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    sw = dict(swk_dense_to_sparse=keys["d2s"], swk_sparse_to_dense=keys["s2d"]) if with_keys else {}
    c.ckks_bootstrap(ct, cs, out, so, plan, cts, stc, keys["conj"], keys["relin"], batch, ws[:need // 8], **sw)
    torch.cuda.synchronize()
    want, ws_stride, _, _ = chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, cs, batch, with_keys)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, ws_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow]), (name, ratio, batch, with_keys)
    assert batch == 1 or not np.array_equal(g[0, :ow], g[1, :ow])
    assert np.all(g[:, room:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"
    assert int(hg.to_host(ws[need // 8:])[0]) == SENT, "the word behind the workspace is intact"


# ---------------------------------------------------------------- 2. encrypted accuracy
def f_of(a, rho):
    return rho / (2 * np.pi) * np.sin(2 * np.pi * a / rho)


def head_message():
    a = np.zeros(N)
    a[:8] = np.array([1.00, -0.50, 0.25, -1.75, 2.50, -3.25, 0.125, -0.875]) / 8  # _head_message() of
    return a                                          # test_gpu_encoding_transform.py scaled into [-0.5, 0.5]


_real = {}


def real(hg, name, sparse_switch):
    """context, plan, keys from a seeded Rng and the encoded factors (kept for the module)"""
    if (name, sparse_switch) in _real:
        return _real[(name, sparse_switch)]
    c, primes = make_context(hg, name)
    plan = hg.bootstrap_plan(primes[:c.Q_size], DELTA, c.Q_size - 1, K=K)
    rng = hg.Rng(2026)
    keys = {}
    if sparse_switch:  # as the reference's example 5: the caller's secret is dense, the raise happens under a sparse one
        sk = c.generate_secret_key(rng)
        sparse = c.generate_secret_key(rng, 32)
        keys["d2s"] = c.generate_switch_key(rng, sparse, sk)
        keys["s2d"] = c.generate_switch_key(rng, sk, sparse)
    else:
        sk = c.generate_secret_key(rng, 32)
    pk = c.generate_public_key(rng, sk)
    keys["relin"] = c.generate_relin_key(rng, sk)
    galois = {}

    def galois_key(e):
        if e not in galois:
            galois[e] = c.generate_galois_key(rng, sk, e)
        return galois[e]
    cts, stc, elts = c.bootstrap_factors(plan, galois_key)
    keys["conj"] = galois_key(2 * N - 1)
    assert sorted(galois) == elts
    _real[(name, sparse_switch)] = (c, primes, plan, rng, sk, pk, keys, cts, stc)
    return _real[(name, sparse_switch)]


def exhausted(c, torch, rng, pk, plain):
    """encrypt and keep the q_0 limb of both parts: a ciphertext at depth Q - 1"""
    ct = c.ckks_encrypt(rng, pk, plain)
    return torch.cat([ct[:N], ct[c.Q_size * N:c.Q_size * N + N]]).contiguous()


def overflow_of_the_raise(hg, torch, c, primes, sk, raised, depth):
    """the integers I of t = k1 D a + q_0 I + e, from the decryption of the raised ciphertext (two limbs hold t)"""
    plain = c.ckks_decrypt(raised, sk, depth=depth)
    two = plain[:2 * N].clone()
    c.ntt(two, two, True, 2, 2)
    torch.cuda.synchronize()
    r = hg.to_host(two).reshape(2, N)
    q0, q1 = primes[0], primes[1]
    inv = pow(q0, -1, q1)
    t = [int(x) + q0 * (((int(y) - int(x)) * inv) % q1) for x, y in zip(r[0], r[1])]
    t = [v - q0 * q1 if v > q0 * q1 // 2 else v for v in t]
    return np.array([(2 * v + q0) // (2 * q0) for v in t], dtype=np.int64), np.array([float(v) for v in t])


def refresh(hg, torch, c, plan, keys, cts, stc, ct):
    room = 2 * (plan.out_level + 2) * N
    out = torch.empty(room, dtype=torch.int64, device="cuda")
    with_keys = "d2s" in keys
    ws = torch.empty(c.bootstrap_workspace_bytes(plan, cts, stc, with_keys, 1) // 8, dtype=torch.int64, device="cuda")
    sw = dict(swk_dense_to_sparse=keys["d2s"], swk_sparse_to_dense=keys["s2d"]) if with_keys else {}
    c.ckks_bootstrap(ct, 2 * N, out, room, plan, cts, stc, keys["conj"], keys["relin"], 1, ws, **sw)
    return out


@pytest.mark.parametrize("which", ["eight_values", "random_all_n"])
@pytest.mark.parametrize("sparse_switch", [False, True], ids=["sparse_secret", "dense_secret_and_switch_keys"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_refreshed_coefficients(hg, torch, name, sparse_switch, which):
    c, primes, plan, rng, sk, pk, keys, cts, stc = real(hg, name, sparse_switch)
    a = head_message() if which == "eight_values" else np.random.default_rng(5).uniform(-0.5, 0.5, N)
    ct = exhausted(c, torch, rng, pk, c.ckks_encode_ex(2, torch.from_numpy(a).cuda(), DELTA))
    # the precondition: the raise entry by entry, decrypted on the host
    _, _, raised, _ = chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, 2 * N, 1, sparse_switch)
    I, t = overflow_of_the_raise(hg, torch, c, primes, sk, raised, c.Q_size - 1 - plan.cts_level)
    rho = primes[0] / (plan.k1 * DELTA)
    raise_err = np.abs(t - primes[0] * I.astype(np.float64) - plan.k1 * DELTA * a).max() / (plan.k1 * DELTA)
    print(f"{name} {which} switch={sparse_switch}: max |I| = {np.abs(I).max()} (K = {K}), deviation {I.std():.2f}, "
          f"|t - q0 I - k1 D a| / (k1 D) = {raise_err:.3e}")
    assert np.abs(I).max() <= K - 1, "an overflow of the raise outside the range EvalMod is built for"
    out = refresh(hg, torch, c, plan, keys, cts, stc, ct)
    depth = c.Q_size - 1 - plan.out_level
    got = c.ckks_decode_ex(2, c.ckks_decrypt(out, sk, depth=depth), plan.out_scale, depth=depth).cpu().numpy()
    err = np.abs(got - f_of(a, rho)).max()
    print(f"{name} {which} switch={sparse_switch}: max |refreshed - f(a)| = {err:.3e} over {N} coefficients (criterion 1e-4); "
          f"against a itself {np.abs(got - a).max():.3e}")
    assert abs(plan.out_scale / DELTA - 1) <= 1e-12
    assert err < 1e-4


def test_refreshed_slots(hg, torch):
    """the reference example's message, 0.2 + 0.4 i in every slot: coefficient 0 is 0.2, coefficient N / 2 is 0.4, so the
    slot-wise image of f is f(0.2) + f(0.4) i"""
    c, primes, plan, rng, sk, pk, keys, cts, stc = real(hg, "A", True)
    z = torch.full((SLOTS,), 0.2 + 0.4j, dtype=torch.complex128, device="cuda")
    ct = exhausted(c, torch, rng, pk, c.ckks_encode_ex(1, z, DELTA))
    out = refresh(hg, torch, c, plan, keys, cts, stc, ct)
    depth = c.Q_size - 1 - plan.out_level
    got = c.ckks_decode_ex(1, c.ckks_decrypt(out, sk, depth=depth), plan.out_scale, depth=depth).cpu().numpy()
    rho = primes[0] / (plan.k1 * DELTA)
    err = np.abs(got - (f_of(0.2, rho) + 1j * f_of(0.4, rho))).max()
    print(f"A slots: max |refreshed - (f(0.2) + f(0.4) i)| = {err:.3e} over {SLOTS} slots (criterion 1e-4)")
    assert err < 1e-4


# ---------------------------------------------------------------- 3. EvalMod alone under encryption
def model(K, degree, r, u):  # tests/test_eval_mod_plan.py
    c = (1.0 / (2.0 * math.pi)) ** (1.0 / 2 ** r)
    coeffs = np.polynomial.chebyshev.chebinterpolate(lambda x: c * np.cos(2 * np.pi * (K * x - 0.25) / 2 ** r), degree)
    y = np.polynomial.chebyshev.chebval(u, coeffs)
    for i in range(r):
        y = 2 * y * y - c ** (2 ** (i + 1))
    return y


@pytest.mark.parametrize("name", ["A", "B"])
def test_eval_mod_under_encryption(hg, torch, name):
    c, primes, plan, rng, sk, pk, keys, cts, stc = real(hg, name, False)
    level = plan.eval_level
    S = float(primes[level])
    em = hg.eval_mod_plan(K, DEGREE, R, level, S, S, primes[:c.Q_size])
    g = np.random.default_rng(9)
    us = []
    for I in range(-(K - 1), K):
        eps = np.concatenate([g.uniform(-2.0 ** -9, 2.0 ** -9, 86), [-2.0 ** -9, 0.0, 2.0 ** -9]])
        us.append((I + eps) / K)
    u = np.concatenate(us)
    u = np.concatenate([u, np.zeros(SLOTS - len(u))])
    assert len(u) == SLOTS and np.abs(u).max() <= 1
    full = c.ckks_encrypt(rng, pk, c.ckks_encode_ex(1, torch.from_numpy(u.astype(np.complex128)).cuda(), S))
    Q, l = c.Q_size, level + 1
    ct = torch.cat([full[:l * N], full[Q * N:Q * N + l * N]]).contiguous()  # the first level + 1 limbs of both parts
    out = torch.empty(2 * em.out_limbs * N, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.poly_eval_workspace_bytes(em, Q - l, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_poly_eval(ct, 2 * l * N, out, 2 * em.out_limbs * N, em, keys["relin"], Q - l, 1, ws)
    depth = Q - 1 - em.level
    got = c.ckks_decode_ex(1, c.ckks_decrypt(out, sk, depth=depth), em.scale, depth=depth).cpu().numpy()
    rho = primes[0] / (plan.k1 * DELTA)
    err = np.abs(got - model(K, DEGREE, R, u)).max()
    print(f"{name} EvalMod under encryption: max |y_r - model| = {err:.3e}, times rho = {err * rho:.3e} (criterion 1e-4)")
    assert err * rho < 1e-4


# ---------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(hg, torch):
    c, primes, plan, cts, stc, keys = synthetic(hg, "A", 256.0)
    Q = c.Q_size
    ct = hg.to_device(synth_ct(primes, [0], 2, N, 1))
    room = 2 * (plan.out_level + 2) * N
    buf = torch.full((2 * room,), SENT, dtype=torch.int64, device="cuda")
    out = buf[:room]
    ws = torch.empty(c.bootstrap_workspace_bytes(plan, cts, stc, True, 1) // 8, dtype=torch.int64, device="cuda")
    both = dict(swk_dense_to_sparse=keys["d2s"], swk_sparse_to_dense=keys["s2d"])

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote its result buffer"

    call = lambda **kw: c.ckks_bootstrap(kw.pop("ct", ct), 2 * N, kw.pop("out", out), room, kw.pop("plan", plan),  # noqa: E731
                                         kw.pop("cts", cts), kw.pop("stc", stc), keys["conj"], keys["relin"],
                                         kw.pop("batch", 1), kw.pop("ws", ws), **kw)
    # exactly one of the two switch keys
    refused(lambda: call(swk_dense_to_sparse=keys["d2s"]))
    refused(lambda: call(swk_sparse_to_dense=keys["s2d"]))
    # batch < 1; a short workspace (with keys it needs the second raised ciphertext)
    refused(lambda: call(batch=0, **both))
    refused(lambda: call(ws=ws[:ws.numel() - 1], **both))
    short = c.bootstrap_workspace_bytes(plan, cts, stc, False, 1) // 8
    assert short < ws.numel()
    refused(lambda: call(ws=ws[:short], **both))
    # a plan that does not fit the context (made for a chain one limb longer), a factor list of the wrong length
    deeper = hg.bootstrap_plan(primes[:Q] + [primes[Q - 1]], DELTA, Q, K=K)
    refused(lambda: call(plan=deeper, **both))
    refused(lambda: call(cts=cts[:2], **both))
    refused(lambda: call(stc=stc + stc[:1], **both))
    # a plan whose EvalMod steps are another plan's
    mixed = hg.BootstrapPlan(plan.c, hg.eval_mod_plan(K, DEGREE, R, plan.eval_level, plan.eval_in_scale, 2.0 ** 49, primes[:Q]))
    refused(lambda: call(plan=mixed, **both))
    # an output overlapping the input or the workspace
    joint = torch.full((2 * N + room,), SENT, dtype=torch.int64, device="cuda")
    refused(lambda: call(ct=joint[:2 * N], out=joint[2 * N - 1:2 * N - 1 + room], **both))
    refused(lambda: call(out=ws[:room], **both))
    torch.cuda.synchronize()
    assert bool((joint == SENT).all())
