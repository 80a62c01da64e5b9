"""CKKS method I, fused key switch: the mod-down as the tail of the row pass + inner product (context option
"moddown_in_mac", ops.cpp ckks_keyswitch_core) against the mod-down row pass of its own (the option at 0), bit for
bit, and against the oracle where a shape is small enough for it.

The new order only runs on the large-launch fused path (no digit splits), so the launch-size rules decide which
batches reach it: at N = 2^16 batches 1 and 2 take the split kernel and 8 and 64 the new order; at N = 2^15 batches 1
and 2 the unfused sequence, 8 and 64 the new order; at N = 2^14 only 64 does.  The remaining shapes check that the
option leaves the other paths alone.  Relinearize works in place (out == ct); apply_galois writes a separate output
through the Galois scatter of the tail."""
import numpy as np
import pytest

from helpers import backend_switches, synth_ct, synth_key

pytestmark = pytest.mark.gpu

CHAINS = {
    14: ([50] + [40] * 7, [50]),   # config C2
    15: ([60] + [50] * 14, [60]),
    16: ([60] + [50] * 15, [60]),  # config C4
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_ctx_cache = {}


def _pair(hg, n_power):
    """two contexts of one chain, moddown_in_mac 0 and 1"""
    if n_power not in _ctx_cache:
        log_q, log_p = CHAINS[n_power]
        cs = []
        for v in (0, 1):
            with backend_switches(HEGPU_MODDOWN_IN_MAC=v):
                c = hg.Context.from_bit_sizes(hg.CKKS, 1 << n_power, log_q, log_p, sec=hg.SEC_NONE)
            assert c.get_option("moddown_in_mac") == v
            c.upload()
            cs.append(c)
        _ctx_cache[n_power] = cs
    return _ctx_cache[n_power]


def _residues(torch, primes, limb_ids, rows, n, gen):
    """[rows][len(limb_ids)][n] uniform residues on the device (row r, limb j below primes[limb_ids[j]])"""
    out = torch.empty((rows, len(limb_ids), n), dtype=torch.int64, device="cuda")
    for j, lid in enumerate(limb_ids):
        out[:, j] = torch.randint(0, primes[lid], (rows, n), generator=gen, device="cuda", dtype=torch.int64)
    return out


def _key(torch, primes, Q, Qp, n, gen):
    k = torch.empty((Q, 2, Qp, n), dtype=torch.int64, device="cuda")
    for j in range(Qp):
        k[:, :, j] = torch.randint(0, primes[j], (Q, 2, n), generator=gen, device="cuda", dtype=torch.int64)
    return k.reshape(-1)


@pytest.mark.parametrize("batch", [1, 2, 8, 64])
@pytest.mark.parametrize("depth", [0, 1, 3])
@pytest.mark.parametrize("n_power", [14, 15, 16])
def test_relinearize_moddown_in_mac_matches_separate_pass(hg, torch, n_power, depth, batch):
    c0, c1 = _pair(hg, n_power)
    n = 1 << n_power
    primes = [int(x) for x in c0.table("modulus")]
    Q, Qp = c0.Q_size, c0.Q_prime_size
    l = Q - depth
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * n_power + 10 * depth + batch)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(l), 3 * batch, n, gen).reshape(batch, 3 * l * n)
    got = []
    for c in (c0, c1):
        x = ct.clone().reshape(-1)
        c.ckks_relinearize_inplace(x, 3 * l * n, key, depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
        torch.cuda.synchronize()
        got.append(x.reshape(batch, 3 * l * n)[:, :2 * l * n])
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("batch", [2, 8, 64])
@pytest.mark.parametrize("n_power,depth", [(14, 0), (15, 1), (16, 0), (16, 3)])
def test_apply_galois_moddown_in_mac_matches_separate_pass(hg, torch, n_power, depth, batch):
    c0, c1 = _pair(hg, n_power)
    n = 1 << n_power
    primes = [int(x) for x in c0.table("modulus")]
    Q, Qp = c0.Q_size, c0.Q_prime_size
    l = Q - depth
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7000 * n_power + 10 * depth + batch)
    key = _key(torch, primes, Q, Qp, n, gen)
    ct = _residues(torch, primes, range(l), 2 * batch, n, gen).reshape(-1)
    for steps in (1, 7, -3):
        g = hg.steps_to_galois_elt(steps, n, 5)
        got = []
        for c in (c0, c1):
            out = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
            c.ckks_apply_galois(ct, 2 * l * n, out, 2 * l * n, key, g, depth, batch,
                                c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
            torch.cuda.synchronize()
            got.append(out)
        assert torch.equal(got[0], got[1]), steps


@pytest.mark.parametrize("n_power,depth", [(14, 0), (14, 1), (15, 3)])
def test_moddown_in_mac_against_oracle(hg, oracle, torch, n_power, depth):
    """The fused path forced for two ciphertexts (no digit splits), so that the oracle can check the new order
    itself: relinearize in place and two rotations."""
    n = 1 << n_power
    log_q, log_p = CHAINS[n_power]
    with backend_switches(HEGPU_FUSED_ROW_MAC=1, HEGPU_DIGIT_SPLIT=0, HEGPU_MODDOWN_IN_MAC=1):
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
