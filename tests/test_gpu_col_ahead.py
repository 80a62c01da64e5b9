"""The modulus loops of the multi-modulus decomposing column pass (ntt_fwd_col_multi<S1>, ntt_fwd_col_decomp_all<8>,
csrc/ntt.hip): what a body reads per target modulus -- the mod-down's "half mod q_j", the digit's own prime for the
choice of the input reduction, the lane's slice of the second-round twiddles -- and which targets the loops execute.
Inside the loops the first two come through the scalar cache and the source registers have landed before the loop on
every path into it, so that nothing at the head of a body waits for the stores of the previous target.  The cases are
chosen for what the loops do per target, not for the workload.  Every case is compared bit for bit

* with the CPU oracle, and
* with the same calls on a context with col_multi = 0: the per-polynomial column kernels, which read
  the same words with plain loads.

One or two ciphertexts each (col_multi forced, a launch this small would take the per-polynomial kernel by itself):

* {60, 50, 50 | 60}, N = 2^16 (ntt_fwd_col_decomp_all<8>): FP64 targets first, then two integer slots.  Digit 0 is the
  wide source and its identity is an integer slot; digits 1 and 2 have their identity in the middle and at the end of
  the FP64 targets.  At depth 1 and 2 three and two targets are left: digits with ONE executed FP64 target, with none
  at all, and both parities of the twiddle buffer at the hand-over to the integer bodies.
* {50, 50, 50 | 50}, N = 2^16 (ntt_fwd_col_multi<8> alone): no integer target, for the last digit the identity is the
  last slot.
* N = 2^13 and 2^14 with the two passes forced (S1 = 5, 6), one chain with and one without integer moduli.
* Fused (FORCED: the source tiles arrive half-way through their inverse transform, src_inv; the mod-down runs inside the
  inner product) and unfused (the mod-down transform is a launch of the column pass of its own: half_on, a wide source,
  T written through decomp_out_mul).  Relinearize and one rotation with a Galois key, batch 1 and 2.
* The same calls a second time on the same buffers."""
import numpy as np
import pytest

from helpers import backend_switches, synth_ct, synth_key

pytestmark = pytest.mark.gpu

INT_LAST = ([60, 50, 50], [60])
NO_INT = ([50, 50, 50], [50])
# the multi-modulus column pass whatever the launch size, and the two passes at every degree
MULTI = dict(HEGPU_COL_MULTI=1, HEGPU_SINGLE_PASS=0)
FORCED = dict(MULTI, HEGPU_FUSED_ROW_MAC=1)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _context(hg, oracle, n, chain, sw):
    log_q, log_p = chain
    with backend_switches(**sw):
        c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    assert (c.Q_size, c.Q_prime_size) == (len(log_q), len(log_q) + len(log_p))
    return c, primes


_wanted = {}


def _reference(hg, oracle, n, chain, depth, primes):
    """two distinct three-part ciphertexts at a depth, their relinearization and its rotation by the oracle: computed
    once per (degree, chain, depth), shared by the cases, never written to"""
    key_id = (n, tuple(chain[0]), tuple(chain[1]), depth)
    if key_id not in _wanted:
        Q, Qp = len(chain[0]), len(chain[0]) + len(chain[1])
        l = Q - depth
        o = oracle.OracleContext(oracle.CKKS, n.bit_length() - 1, primes, Q, Qp - Q)
        g = hg.steps_to_galois_elt(1, n, 5)
        key, gkey = synth_key(primes, Q, Qp, n, 3), synth_key(primes, Q, Qp, n, 4)
        cts, relin, rot = [], [], []
        for b in range(2):
            ct = synth_ct(primes, range(l), 3, n, 5 + 10 * b + 100 * depth)
            r = o.ckks_relinearize(ct.copy(), key, depth)[:2 * l * n].copy()
            cts.append(ct)
            relin.append(r)
            rot.append(o.ckks_apply_galois(r.copy(), gkey, g, depth))
        for x in cts + relin + rot:
            x.setflags(write=False)
        _wanted[key_id] = (g, key, gkey, cts, relin, rot)
    return _wanted[key_id]


def _run(hg, torch, c, n, l, depth, g, key, gkey, cts, batch, rounds):
    """relinearize in place, then rotate; `rounds` times on the same device buffers and workspaces.  Returns the
    results of every round."""
    src = np.concatenate([cts[b % 2] for b in range(batch)])
    d = hg.to_device(src)
    out = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
    dkey, dgkey = hg.to_device(key), hg.to_device(gkey)
    ws_r, ws_g = c.workspace(hg.OP_CKKS_RELIN, depth, batch), c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
    got = []
    for _ in range(rounds):
        d.copy_(hg.to_device(src))
        c.ckks_relinearize_inplace(d, 3 * l * n, dkey, depth, batch, ws_r)
        c.ckks_apply_galois(d, 3 * l * n, out, 2 * l * n, dgkey, g, depth, batch, ws_g)
        torch.cuda.synchronize()
        got.append((hg.to_host(d).reshape(batch, -1)[:, :2 * l * n].copy(), hg.to_host(out).reshape(batch, -1).copy()))
    return got


def _check(hg, oracle, torch, n, chain, sw, depth, batch, rounds=1):
    c, primes = _context(hg, oracle, n, chain, sw)
    l = len(chain[0]) - depth
    g, key, gkey, cts, relin, rot = _reference(hg, oracle, n, chain, depth, primes)
    got = _run(hg, torch, c, n, l, depth, g, key, gkey, cts, batch, rounds)
    for r, (got_relin, got_rot) in enumerate(got):
        for b in range(batch):
            assert np.array_equal(got_relin[b], relin[b % 2]), ("relinearize against the oracle", r, b)
            assert np.array_equal(got_rot[b], rot[b % 2]), ("rotate against the oracle", r, b)
    # the per-polynomial column kernels under otherwise the same switches
    c0, primes0 = _context(hg, oracle, n, chain, dict(sw, HEGPU_COL_MULTI=0))
    assert primes0 == primes
    (ref_relin, ref_rot), = _run(hg, torch, c0, n, l, depth, g, key, gkey, cts, batch, 1)
    for got_relin, got_rot in got:
        assert np.array_equal(got_relin, ref_relin), "relinearize against col_multi = 0"
        assert np.array_equal(got_rot, ref_rot), "rotate against col_multi = 0"


@pytest.mark.parametrize("sw", [FORCED, MULTI], ids=["fused_src_inv", "unfused_moddown_launch"])
@pytest.mark.parametrize("batch", [1, 2])
def test_integer_targets_last(hg, oracle, torch, sw, batch):
    _check(hg, oracle, torch, 65536, INT_LAST, sw, 0, batch)


@pytest.mark.parametrize("sw", [FORCED, MULTI], ids=["fused_src_inv", "unfused_moddown_launch"])
def test_no_integer_target(hg, oracle, torch, sw):
    _check(hg, oracle, torch, 65536, NO_INT, sw, 0, 2)


@pytest.mark.parametrize("chain", [INT_LAST, NO_INT], ids=["integer_last", "no_integer"])
@pytest.mark.parametrize("depth", [1, 2])
def test_short_chains(hg, oracle, torch, chain, depth):
    """three, then two targets per digit: one executed target or none after the identity skip"""
    _check(hg, oracle, torch, 65536, chain, FORCED, depth, 2)


@pytest.mark.parametrize("chain", [INT_LAST, NO_INT], ids=["integer_last", "no_integer"])
@pytest.mark.parametrize("n", [8192, 16384])
def test_smaller_degrees(hg, oracle, torch, n, chain):
    """S1 = 5 and 6 (ntt_fwd_col_multi<S1>; integer targets by the per-polynomial kernel), at depth 0 and 1"""
    _check(hg, oracle, torch, n, chain, FORCED, 0, 2)
    _check(hg, oracle, torch, n, chain, MULTI, 1, 1)


@pytest.mark.parametrize("chain", [INT_LAST, NO_INT], ids=["integer_last", "no_integer"])
def test_same_call_twice(hg, oracle, torch, chain):
    _check(hg, oracle, torch, 65536, chain, FORCED, 0, 2, rounds=2)
