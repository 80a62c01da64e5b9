"""Fused key switch, launches without digit splits: the wide row kernels (context option "wide_access", ntt.hip
ks_pair_mac_fp / ks_pair_mac, KsMacArgs::wide) against the natural forms (the option at 0), bit for bit, and against
the oracle where a shape is small enough for it.

The wide forms only change which lane holds which element past the row stages (tests/test_wide_layout_model.py), so
every output must be equal.  Two contexts per chain, option 0 and 1, in the style of tests/test_gpu_moddown_in_mac.py.
The launch-size rules decide which batches reach the fused path without splits: at N = 2^16 batches 8 and up, at
N = 2^15 batch 8, at N = 2^14 batch 64; smaller launches are forced there through the context options or show that the
option leaves the split and the unfused paths alone.  Covered: the FP64 and the integer kernels with the mod-down tail
(CKKS relinearize in place, rotations through the Galois scatter of the tail), without it (BFV), a chain whose moduli
all take the integer butterflies, the identity limb, and an evaluation key or a ciphertext that is not 16-byte aligned
(the launch falls back to the natural forms).  Equal outputs alone would also pass if the wide kernels never ran, so the
cases count the launches by form (hg.ks_launch_forms: natural, wide, split) around each call."""
import numpy as np
import pytest

from helpers import backend_switches, synth_ct, synth_key

pytestmark = pytest.mark.gpu

CHAINS = {
    14: ([50] + [40] * 7, [50]),   # config C2
    15: ([60] + [50] * 14, [60]),
    16: ([60] + [50] * 15, [60]),  # config C4
}
FORCED = dict(fused_row_mac=1, digit_split=0, col_multi=1)
UNFORCED = dict(fused_row_mac=-1, digit_split=-1, col_multi=-1)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_ctx_cache = {}


def _pair(hg, n_power):
    """two contexts of one chain, wide_access 0 and 1"""
    if n_power not in _ctx_cache:
        log_q, log_p = CHAINS[n_power]
        cs = []
        for v in (0, 1):
            with backend_switches(HEGPU_WIDE_ACCESS=v):
                c = hg.Context.from_bit_sizes(hg.CKKS, 1 << n_power, log_q, log_p, sec=hg.SEC_NONE)
            assert c.get_option("wide_access") == v
            c.upload()
            cs.append(c)
        _ctx_cache[n_power] = cs
    return _ctx_cache[n_power]


def _force(pair, forced):
    for c in pair:
        for k, v in (FORCED if forced else UNFORCED).items():
            c.set_option(k, v)


def _residues(torch, primes, limb_ids, rows, n, gen):
    out = torch.empty((rows, len(limb_ids), n), dtype=torch.int64, device="cuda")
    for j, lid in enumerate(limb_ids):
        out[:, j] = torch.randint(0, primes[lid], (rows, n), generator=gen, device="cuda", dtype=torch.int64)
    return out


def _key(torch, primes, Q, Qp, n, gen, lead=0):
    """evaluation key; lead: elements in front of it in its buffer (1: the key starts 8 bytes off a 16-byte boundary)"""
    buf = torch.empty(lead + Q * 2 * Qp * n, dtype=torch.int64, device="cuda")
    k = buf[lead:].view(Q, 2, Qp, n)
    for j in range(Qp):
        k[:, :, j] = torch.randint(0, primes[j], (Q, 2, n), generator=gen, device="cuda", dtype=torch.int64)
    return buf[lead:]


def test_option_defaults_to_one_and_is_cloned(hg):
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [40, 30, 30], [40], sec=hg.SEC_NONE)
    assert c.get_option("wide_access") == 1
    c.set_option("wide_access", 0)
    assert c.clone().get_option("wide_access") == 0
    with pytest.raises(Exception):
        c.set_option("wide_access", 2)


def _forms(hg, call):
    """(natural, wide, split) launches of the fused row pass made by call()"""
    before = hg.ks_launch_forms()
    call()
    return tuple(b - a for a, b in zip(before, hg.ks_launch_forms()))


def _check_forms(forms, fused):
    """forms: per context (option 0, option 1).  fused (without splits): option 0 launches the natural kernels only,
    option 1 the wide ones only; else neither context reaches either (split kernel, or no fused launch at all)"""
    (n0, w0, s0), (n1, w1, s1) = forms
    if fused:
        assert n0 > 0 and w0 == 0 and s0 == 0, forms
        assert w1 == n0 and n1 == 0 and s1 == 0, forms
    else:
        assert n0 == w0 == n1 == w1 == 0 and s0 == s1, forms


# (n_power, depth, batch, forced, fused): the fused path without splits by launch size, forced for a small launch with
# the multi-modulus column pass, and launches that stay on the split (2^16) / unfused (2^15) paths
RELIN_CASES = [(16, 0, 8, False, True), (16, 3, 2, True, True), (15, 0, 8, False, True), (14, 0, 64, False, True),
               (16, 0, 1, False, False), (16, 0, 2, False, False), (15, 0, 2, False, False)]


@pytest.mark.parametrize("n_power,depth,batch,forced,fused", RELIN_CASES)
def test_relinearize_wide_matches_natural(hg, torch, n_power, depth, batch, forced, fused):
    pair = _pair(hg, n_power)
    _force(pair, forced)
    n = 1 << n_power
    primes = [int(x) for x in pair[0].table("modulus")]
    Q, Qp = pair[0].Q_size, pair[0].Q_prime_size
    l = Q - depth
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1100 * n_power + 10 * depth + batch)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(l), 3 * batch, n, gen).reshape(batch, 3 * l * n)
    got, forms = [], []
    for c in pair:
        x = ct.clone().reshape(-1)
        ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
        forms.append(_forms(hg, lambda: c.ckks_relinearize_inplace(x, 3 * l * n, key, depth, batch, ws)))
        torch.cuda.synchronize()
        got.append(x.reshape(batch, 3 * l * n)[:, :2 * l * n])
    _force(pair, False)
    assert torch.equal(got[0], got[1])
    _check_forms(forms, fused)


@pytest.mark.parametrize("n_power,depth,batch,forced", [(16, 0, 8, False), (16, 3, 2, True), (15, 1, 8, False), (14, 0, 64, False)])
def test_apply_galois_wide_matches_natural(hg, torch, n_power, depth, batch, forced):
    """the Galois scatter of the tail with the element index of the pair ownership"""
    pair = _pair(hg, n_power)
    _force(pair, forced)
    n = 1 << n_power
    primes = [int(x) for x in pair[0].table("modulus")]
    Q, Qp = pair[0].Q_size, pair[0].Q_prime_size
    l = Q - depth
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7100 * n_power + 10 * depth + batch)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(l), 2 * batch, n, gen).reshape(-1)
    res, forms = {}, {}
    for steps in (1, 7, -3):
        g = hg.steps_to_galois_elt(steps, n, 5)
        got, forms[steps] = [], []
        for c in pair:
            out = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
            ws = c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
            forms[steps].append(_forms(hg, lambda: c.ckks_apply_galois(ct, 2 * l * n, out, 2 * l * n, key, g, depth, batch, ws)))
            torch.cuda.synchronize()
            got.append(out)
        res[steps] = bool(torch.equal(got[0], got[1]))
    _force(pair, False)
    assert all(res.values()), res
    for steps in forms:
        _check_forms(forms[steps], True)


def test_unaligned_key_takes_the_natural_forms(hg, torch):
    """a key 8 bytes off a 16-byte boundary: the wide launch falls back, same residues as with the aligned copy"""
    n_power, depth, batch = 14, 0, 64
    pair = _pair(hg, n_power)
    c = pair[1]
    n = 1 << n_power
    primes = [int(x) for x in c.table("modulus")]
    Q, Qp = c.Q_size, c.Q_prime_size
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    odd = _key(torch, primes, Q, Qp, n, gen, lead=1)
    assert odd.data_ptr() % 16 == 8
    even = odd.clone()
    assert even.data_ptr() % 16 == 0
    ct = _residues(torch, primes, range(Q), 3 * batch, n, gen).reshape(-1)
    got, forms = [], []
    for key in (even, odd):
        x = ct.clone()
        ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
        forms.append(_forms(hg, lambda: c.ckks_relinearize_inplace(x, 3 * Q * n, key, depth, batch, ws)))
        torch.cuda.synchronize()
        got.append(x.reshape(batch, 3 * Q * n)[:, :2 * Q * n])
    assert torch.equal(got[0], got[1])
    (n_e, w_e, s_e), (n_o, w_o, s_o) = forms
    assert w_e > 0 and n_e == 0 and n_o == w_e and w_o == 0 and s_e == s_o == 0, forms


def test_unaligned_ciphertext_takes_the_natural_forms(hg, torch):
    """the ciphertext (source of the identity limb, added term and output of the in-place call) 8 bytes off a 16-byte
    boundary: every launch of the call falls back, same residues as with the aligned copy"""
    n_power, depth, batch = 14, 0, 64
    c = _pair(hg, n_power)[1]
    n = 1 << n_power
    primes = [int(x) for x in c.table("modulus")]
    Q, Qp = c.Q_size, c.Q_prime_size
    gen = torch.Generator(device="cuda")
    gen.manual_seed(98)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(Q), 3 * batch, n, gen).reshape(-1)
    buf = torch.empty(ct.numel() + 1, dtype=torch.int64, device="cuda")
    got, forms = [], []
    for lead in (0, 1):
        x = buf[lead:lead + ct.numel()]
        x.copy_(ct)
        assert x.data_ptr() % 16 == 8 * lead
        ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
        forms.append(_forms(hg, lambda: c.ckks_relinearize_inplace(x, 3 * Q * n, key, depth, batch, ws)))
        torch.cuda.synchronize()
        got.append(x.reshape(batch, 3 * Q * n)[:, :2 * Q * n].clone())
    assert torch.equal(got[0], got[1])
    (n_e, w_e, s_e), (n_o, w_o, s_o) = forms
    assert w_e > 0 and n_e == 0 and n_o > 0 and w_o == 0 and s_e == s_o == 0, forms


def _two(hg, make):
    cs = []
    for v in (0, 1):
        with backend_switches(HEGPU_WIDE_ACCESS=v, HEGPU_FUSED_ROW_MAC=1, HEGPU_DIGIT_SPLIT=0):
            c = make()
        assert c.get_option("wide_access") == v
        c.upload()
        cs.append(c)
    return cs


def test_bfv_relinearize_wide_matches_natural(hg, torch):
    """no mod-down tail: the plain 16-byte output stores of the wide forms (fused path forced for two ciphertexts)"""
    n = 1 << 14
    cs = _two(hg, lambda: hg.Context.from_default(hg.BFV, n, 1, 786433))
    primes = [int(x) for x in cs[0].table("modulus")]
    Q, Qp = cs[0].Q_size, cs[0].Q_prime_size
    batch = 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(Q), 3 * batch, n, gen).reshape(-1)
    got, forms = [], []
    for c in cs:
        x = ct.clone()
        ws = c.workspace(hg.OP_BFV_RELIN, 0, batch)
        forms.append(_forms(hg, lambda: c.bfv_relinearize_inplace(x, 3 * Q * n, key, batch, ws)))
        torch.cuda.synchronize()
        got.append(x.reshape(batch, 3 * Q * n)[:, :2 * Q * n])
    assert torch.equal(got[0], got[1])
    _check_forms(forms, True)


def test_integer_only_chain_wide_matches_natural(hg, torch):
    """a 59/58-bit chain at N = 2^14: every modulus on the integer butterflies (no FP64 kernel is launched)"""
    n = 1 << 14
    cs = _two(hg, lambda: hg.Context.from_bit_sizes(hg.CKKS, n, [59] + [58] * 5, [59], sec=hg.SEC_NONE))
    primes = [int(x) for x in cs[0].table("modulus")]
    assert min(primes) >= 1 << 50, "the chain has FP64 moduli: not the case this test is for"
    Q, Qp = cs[0].Q_size, cs[0].Q_prime_size
    batch = 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(41)
    key = _key(torch, primes, Q, Qp, n, gen)
    for depth in (0, 2):
        l = Q - depth
        ct = _residues(torch, primes, range(l), 3 * batch, n, gen).reshape(-1)
        got, rot = [], []
        g = hg.steps_to_galois_elt(3, n, 5)
        for c in cs:
            x = ct.clone()
            c.ckks_relinearize_inplace(x, 3 * l * n, key, depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
            src = ct.reshape(batch, 3 * l * n)[:, :2 * l * n].contiguous().reshape(-1)
            out = torch.empty_like(src)
            c.ckks_apply_galois(src, 2 * l * n, out, 2 * l * n, key, g, depth, batch,
                                c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
            torch.cuda.synchronize()
            got.append(x.reshape(batch, 3 * l * n)[:, :2 * l * n])
            rot.append(out)
        assert torch.equal(got[0], got[1]), depth
        assert torch.equal(rot[0], rot[1]), depth


@pytest.mark.parametrize("n_power,depth", [(14, 0), (14, 1), (15, 3)])
def test_wide_access_against_oracle(hg, oracle, torch, n_power, depth):
    """The fused path forced for two ciphertexts (no digit splits), so that the oracle can check the wide forms
    themselves: relinearize in place and two rotations."""
    n = 1 << n_power
    log_q, log_p = CHAINS[n_power]
    with backend_switches(HEGPU_FUSED_ROW_MAC=1, HEGPU_DIGIT_SPLIT=0, HEGPU_WIDE_ACCESS=1):
        c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    Q, Qp = len(log_q), len(log_q) + len(log_p)
    o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, Q, len(log_p))
    c.upload()
    l = Q - depth
    batch = 2
    key = synth_key(primes, Q, Qp, n, 3)
    gkey = synth_key(primes, Q, Qp, n, 5)
    ct = [synth_ct(primes, range(l), 3, n, 1 + 10 * b) for b in range(batch)]
    d = hg.to_device(np.concatenate(ct))
    c.ckks_relinearize_inplace(d, 3 * l * n, hg.to_device(key), depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
    torch.cuda.synchronize()
    got = hg.to_host(d).reshape(batch, -1)
    for b in range(batch):
        want = o.ckks_relinearize(ct[b].copy(), key, depth)
        assert np.array_equal(got[b][:2 * l * n], want[:2 * l * n]), "relinearize"
    src = [x[:2 * l * n] for x in ct]
    ds = hg.to_device(np.concatenate(src))
    for steps in (1, -5):
        g = hg.steps_to_galois_elt(steps, n, 5)
        rot = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
        c.ckks_apply_galois(ds, 2 * l * n, rot, 2 * l * n, hg.to_device(gkey), g, depth, batch,
                            c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
        torch.cuda.synchronize()
        got_r = hg.to_host(rot).reshape(batch, -1)
        for b in range(batch):
            assert np.array_equal(got_r[b], o.ckks_apply_galois(src[b].copy(), gkey, g, depth)), ("rotate", steps)
