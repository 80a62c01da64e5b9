"""The decomposing column pass with the integer targets in it (ntt_fwd_col_decomp_all<8>, csrc/ntt.hip), bit for bit
against the oracle.  N = 2^16 throughout: the only degree with eight column stages, the only one the kernel is built for.

A launch takes the kernel when it goes through the multi-modulus column pass, the plan has FP64 and integer moduli and the
caller lists the integer target slots -- the digits of a method-I key switch and its mod-down transform (the P limb at
every q_j, NttArgs::half_on).  The multi-modulus pass is chosen by launch size (2048 source tiles) or by the option
col_multi; with the fused row pass + inner product the source tiles also arrive half-way through their inverse transform
(NttArgs::src_inv), and the kernel no longer stores the finished tile.  The chains are short so that a case stays at a few
seconds; what they cover of the kernel:

* {60, 50, 50 | 60}: a wide (u64) source digit 0 and 50-bit sources held as doubles and converted back, two FP64 and two
  integer targets, the identity skip on q0, the 60-bit moduli on the correcting butterflies with room 16;
* {60, 50, 60, 50 | 60}: an integer target between FP64 ones in the order, an identity skip on an integer modulus that is
  not digit 0, two wide sources;
* {50, 50, 50 | 50}: no integer target at all -- the launch rule leaves these launches to ntt_fwd_col_multi<8> alone (what
  a test can see of that is that the results stay right; the budgets test checks that the kernel is still built)."""
import numpy as np
import pytest

from helpers import backend_switches, extreme_limbs, synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 65536
SHORT = ([60, 50, 50], [60])
MIXED = ([60, 50, 60, 50], [60])
NO_INT = ([50, 50, 50], [50])
# the multi-modulus column pass and the fused row pass + inner product whatever the launch size: the source tiles of the
# digits come half-inverted (src_inv), the mod-down runs inside the inner product
FORCED = dict(HEGPU_COL_MULTI=1, HEGPU_FUSED_ROW_MAC=1)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _context(hg, oracle, chain, sw):
    log_q, log_p = chain
    with backend_switches(**sw):
        c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
    c.upload()
    assert (c.Q_size, c.Q_prime_size) == (len(log_q), len(log_q) + len(log_p))
    return c, o, primes


_wanted = {}


def _reference(o, primes, chain, g):
    """two distinct three-part ciphertexts of a chain, their relinearization and its rotation by the oracle: computed
    once per chain, shared by the cases, never written to"""
    key_id = (tuple(chain[0]), tuple(chain[1]))
    if key_id not in _wanted:
        Q, Qp = len(chain[0]), len(chain[0]) + len(chain[1])
        key, gkey = synth_key(primes, Q, Qp, N, 3), synth_key(primes, Q, Qp, N, 4)
        cts, relin, rot = [], [], []
        for b in range(2):
            ct = synth_ct(primes, range(Q), 3, N, 5 + 10 * b)
            r = o.ckks_relinearize(ct.copy(), key, 0)[:2 * Q * N].copy()
            cts.append(ct)
            relin.append(r)
            rot.append(o.ckks_apply_galois(r.copy(), gkey, g, 0))
        for x in cts + relin + rot:
            x.setflags(write=False)
        _wanted[key_id] = (key, gkey, cts, relin, rot)
    return _wanted[key_id]


def _relinearize_and_rotate(hg, oracle, torch, chain, sw, batch):
    c, o, primes = _context(hg, oracle, chain, sw)
    Q = len(chain[0])
    g = hg.steps_to_galois_elt(1, N, 5)
    key, gkey, cts, relin, rot = _reference(o, primes, chain, g)
    d = hg.to_device(np.concatenate([cts[b % 2] for b in range(batch)]))
    c.ckks_relinearize_inplace(d, 3 * Q * N, hg.to_device(key), 0, batch, c.workspace(hg.OP_CKKS_RELIN, 0, batch))
    torch.cuda.synchronize()
    got = hg.to_host(d).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b][:2 * Q * N], relin[b % 2]), ("relinearize", b)
    out = torch.empty(batch * 2 * Q * N, dtype=torch.int64, device="cuda")
    c.ckks_apply_galois(d, 3 * Q * N, out, 2 * Q * N, hg.to_device(gkey), g, 0, batch,
                        c.workspace(hg.OP_CKKS_GALOIS, 0, batch))
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], rot[b % 2]), ("rotate", b)


@pytest.mark.parametrize("sw", [dict(), FORCED], ids=["by_launch_size", "col_multi_fused"])
def test_short_chain_eight_ciphertexts(hg, oracle, torch, sw):
    """Eight ciphertexts: the smallest batch with the launch forms of the bench around the column pass (the inner
    product not split over the digits, the mod-down inside it), so the P-limb launch (half_on, two source tiles per
    ciphertext, one integer target) runs as well as the digits' launch.  By launch size alone these 384 source tiles
    stay with the per-polynomial kernel; the forced case puts the same eight through the new one."""
    _relinearize_and_rotate(hg, oracle, torch, SHORT, sw, 8)


@pytest.mark.parametrize("sw,batch", [(dict(HEGPU_COL_MULTI=1), 1), (dict(HEGPU_COL_MULTI=1), 2), (FORCED, 2)],
                         ids=["one_unfused", "two_unfused", "two_fused"])
def test_short_chain_forced_col_multi(hg, oracle, torch, sw, batch):
    """One and two ciphertexts with the multi-modulus column pass forced.  Launches this small take the unfused key
    switch: the kernel reads finished coefficient-domain limbs (no src_inv) and is followed by the stand-alone row pass;
    the mod-down transform carries its epilogue.  The last case forces the fused path on two."""
    _relinearize_and_rotate(hg, oracle, torch, SHORT, sw, batch)


def test_mixed_chain_integer_target_inside_the_order(hg, oracle, torch):
    _relinearize_and_rotate(hg, oracle, torch, MIXED, FORCED, 2)


def test_extreme_inputs(hg, oracle, torch):
    """The lazy and the correcting integer stages fed from doubles converted back: every residue q - 1 (in the NTT
    domain, and in the coefficient domain so that the digits themselves are q - 1), all zero, one random ciphertext,
    against a key of all q - 1."""
    c, o, primes = _context(hg, oracle, SHORT, FORCED)
    Q, Qp = 3, 4
    key = np.concatenate([np.full(N, primes[j] - 1, dtype=np.uint64) for _ in range(Q) for _c in range(2) for j in range(Qp)])
    pats = ["max", "max_coeff", "zero", "random"]
    cts = []
    for i, pat in enumerate(pats):
        if pat == "zero":
            cts.append(np.zeros(3 * Q * N, dtype=np.uint64))
        else:
            cts.append(np.concatenate([extreme_limbs(c, primes, range(Q), N, pat, 31 * i + p) for p in range(3)]))
    d = hg.to_device(np.concatenate(cts))
    c.ckks_relinearize_inplace(d, 3 * Q * N, hg.to_device(key), 0, len(cts), c.workspace(hg.OP_CKKS_RELIN, 0, len(cts)))
    torch.cuda.synchronize()
    got = hg.to_host(d).reshape(len(cts), -1)
    for b, pat in enumerate(pats):
        want = o.ckks_relinearize(cts[b].copy(), key, 0)
        assert np.array_equal(got[b][:2 * Q * N], want[:2 * Q * N]), pat


def test_chain_without_integer_targets(hg, oracle, torch):
    _relinearize_and_rotate(hg, oracle, torch, NO_INT, FORCED, 2)
