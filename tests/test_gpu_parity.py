"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle, bit-exact.

Shapes follow BASELINE.json configs C1 (BFV N=2^12 default chain) and C2
(CKKS N=2^14, Q=8, P=1); the NTT is covered for every supported N.
"""
import os

import numpy as np
import pytest

from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _ckks_pair(hg, oracle, n, log_q, log_p, sec=None):
    c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_128 if sec is None else sec)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
    c.upload()
    return c, o, primes


def _bfv_pair(hg, oracle, n, t):
    c = hg.Context.from_default(hg.BFV, n, 1, t)
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, t)
    c.upload()
    return c, o, primes


@pytest.mark.parametrize("n_power", [12, 13, 14, 15, 16])
def test_ntt_forward_inverse(hg, oracle, torch, n_power):
    n = 1 << n_power
    # 60/30/45-bit primes exercise the extreme modulus sizes
    c, o, primes = _ckks_pair(hg, oracle, n, [60, 30, 45], [60], sec=hg.SEC_NONE)
    Qp = 4
    batch = 2 * Qp + 4  # wraps around the modulus list
    x = np.concatenate([oracle.fill_poly(7 + i, i % Qp, n, primes[i % Qp]) for i in range(batch)])
    want = o.ntt(x.copy(), batch, Qp)
    d = hg.to_device(x)
    out = torch.empty_like(d)
    c.ntt(d, out, False, batch, Qp)            # GPU_NTT (out of place)
    torch.cuda.synchronize()
    got = hg.to_host(out)
    assert np.array_equal(got, want)
    c.ntt(out, out, True, batch, Qp)           # GPU_INTT_Inplace
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(out), x)
    # inverse vs oracle on arbitrary canonical input
    want_i = o.ntt(x.copy(), batch, Qp, inverse=True)
    c.ntt(d, d, True, batch, Qp)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want_i)


@pytest.mark.parametrize("n_power", [12, 16])
def test_ntt_fp64_path_extremes(hg, oracle, torch, n_power):
    """Forward transform of the moduli that take the FP64 butterflies (< 2^50) next to the
    integer ones (51 bits and up), on the inputs that maximise intermediate magnitudes:
    all q-1, all zero, alternating 0 / q-1, a single q-1, random."""
    n = 1 << n_power
    bits = [50, 50, 49, 36, 51, 57]
    c, o, primes = _ckks_pair(hg, oracle, n, bits, [58], sec=hg.SEC_NONE)
    Qp = len(bits) + 1
    rows = []
    for m in range(Qp):
        q = int(primes[m])
        rows.append(np.full(n, q - 1, dtype=np.uint64))
        rows.append(np.zeros(n, dtype=np.uint64))
        alt = np.zeros(n, dtype=np.uint64); alt[::2] = q - 1
        rows.append(alt)
        one = np.zeros(n, dtype=np.uint64); one[n - 1] = q - 1
        rows.append(one)
        rows.append(oracle.fill_poly(1000 + m, m, n, q))
    # layout for the batched call: polynomial i uses modulus i % Qp
    per = len(rows) // Qp
    x = np.concatenate([rows[(i % Qp) * per + i // Qp] for i in range(per * Qp)])
    want = o.ntt(x.copy(), per * Qp, Qp)
    d = hg.to_device(x)
    c.ntt(d, d, False, per * Qp, Qp)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)
    c.ntt(d, d, True, per * Qp, Qp)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), x)


def test_ntt_bsk_61bit_and_offsets(hg, oracle, torch):
    """61-bit Bsk primes (merged q|Bsk tables) and caller-offset tables."""
    c, o, primes = _bfv_pair(hg, oracle, 4096, 1032193)
    n = 4096
    mm = [int(v) for v in c.table("q_Bsk_merge_modulus")]
    L = len(mm)
    x = np.concatenate([oracle.fill_poly(3 + i, i, n, mm[i % L]) for i in range(2 * L)])
    tab = o.table("q_Bsk_merge_ntt_tables")
    mods = o.mods(mm)
    want = x.copy()
    o.L.o_gpu_ntt(want.ctypes.data, want.ctypes.data, tab.ctypes.data, mods, 12, 2 * L, L)
    d = hg.to_device(x)
    c.ntt(d, d, False, 2 * L, L, table_set=hg.TABLES_Q_BSK)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)
    c.ntt(d, d, True, 2 * L, L, table_set=hg.TABLES_Q_BSK)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), x)
    # mod_offset: transform 2 polys with the P prime only (index Q)
    y = np.concatenate([oracle.fill_poly(50 + i, 2, n, primes[2]) for i in range(2)])
    want = o.ntt(y.copy(), 2, 1, mod_offset=2)
    d = hg.to_device(y)
    c.ntt(d, d, False, 2, 1, mod_offset=2)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)


def test_ntt_ordered_variants(hg, oracle, torch):
    c, o, primes = _ckks_pair(hg, oracle, 8192, [40, 35, 35, 35], [40])
    n, Q, Qp = 8192, 4, 5
    depth = 1
    rc = Qp - depth
    order_host = [int(v) for v in o.table("new_prime_locations")]
    off = Qp  # slice for depth 1 starts at sum_{j<1}(Q'-j)
    order = order_host[off:off + rc]
    batch = 3 * rc
    x = np.concatenate([oracle.fill_poly(11 + i, 0, n, primes[order[i % rc]]) for i in range(batch)])
    tab = o.table("ntt_table")
    ninv = o.table("n_inverse")
    want = x.copy()
    ord_arr = np.array(order, dtype=np.int32)
    o.L.o_gpu_ntt_modulus_ordered(want.ctypes.data, tab.ctypes.data, o.qp_mods, ninv.ctypes.data, 0, 13, batch, rc,
                                  ord_arr.ctypes.data)
    d = hg.to_device(x)
    dev_order = c.device_ptr("new_prime_locations") + 4 * off
    c.ntt(d, d, False, batch, rc, mod_order=dev_order)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)
    # inverse, modulus ordered (apply_galois path, ckks/operator.cu:1524)
    itab = o.table("intt_table")
    o.L.o_gpu_ntt_modulus_ordered(want.ctypes.data, itab.ctypes.data, o.qp_mods, ninv.ctypes.data, 1, 13, batch, rc,
                                  ord_arr.ctypes.data)
    c.ntt(d, d, True, batch, rc, mod_order=dev_order)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)
    assert np.array_equal(want, x)
    # poly ordered: INTT only slots {rc-1, 2rc-1} with the P prime (relin path)
    slots = np.array([rc - 1, 2 * rc - 1], dtype=np.int32)
    z = np.concatenate([oracle.fill_poly(90 + i, 0, n, primes[Qp - 1]) for i in range(2 * rc)])
    want = z.copy()
    o.L.o_gpu_ntt_poly_ordered(want.ctypes.data, itab.ctypes.data + Q * n * 8, o.mods_addr(Q),
                               ninv.ctypes.data + Q * 8, 1, 13, 2, 1, slots.ctypes.data)
    d = hg.to_device(z)
    dev_slots = c.device_ptr("new_input_locations") + 4 * 2 * depth
    c.ntt(d, d, True, 2, 1, mod_offset=Q, poly_order=dev_slots)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(d), want)


def test_add_sub_neg(hg, oracle, torch):
    c, o, primes = _bfv_pair(hg, oracle, 4096, 1032193)
    n, Q = 4096, 2
    batch = 3
    a = np.concatenate([synth_ct(primes, range(Q), 2, n, 1 + b) for b in range(batch)])
    b_ = np.concatenate([synth_ct(primes, range(Q), 2, n, 40 + b) for b in range(batch)])
    a[5] = 0  # negation of zero
    da, db = hg.to_device(a), hg.to_device(b_)
    out = torch.empty_like(da)
    for op, fn in ((0, o.L.o_addition), (1, o.L.o_substraction)):
        want = np.zeros_like(a)
        per = 2 * Q * n
        for i in range(batch):
            fn(a[i * per:].ctypes.data, b_[i * per:].ctypes.data, want[i * per:].ctypes.data, o.qp_mods, 12, Q, 2)
        c.addition(da, db, out, Q, 2, batch, op)
        torch.cuda.synchronize()
        assert np.array_equal(hg.to_host(out), want)
    want = np.zeros_like(a)
    per = 2 * Q * n
    for i in range(batch):
        o.L.o_negation(a[i * per:].ctypes.data, want[i * per:].ctypes.data, o.qp_mods, 12, Q, 2)
    c.addition(da, None, out, Q, 2, batch, 2)
    torch.cuda.synchronize()
    assert np.array_equal(hg.to_host(out), want)


@pytest.mark.parametrize("batch", [1, 2], ids=["batch1", "batch2"])
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_ckks_mul_relin_rescale(hg, oracle, torch, depth, batch):
    """Config C2: CKKS N=2^14, Q{50,40x7} P{50}: multiply -> relinearize -> rescale.  Batch 1 is the configuration
    itself (the launch-size rules pick other kernels there than at batch 2: the unfused key switch, the copy riding on
    the per-polynomial column pass)."""
    n = 16384
    c, o, primes = _ckks_pair(hg, oracle, n, [50] + [40] * 7, [50])
    Q, Qp = 8, 9
    l = Q - depth
    key = synth_key(primes, Q, Qp, n, 3)
    dkey = hg.to_device(key)
    ct1 = [synth_ct(primes, range(l), 2, n, 1 + 10 * b) for b in range(batch)]
    ct2 = [synth_ct(primes, range(l), 2, n, 2 + 10 * b) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * l * n, dtype=torch.int64, device="cuda")
    c.ckks_multiply(d1, 2 * l * n, d2, 2 * l * n, out, 3 * l * n, depth, batch)
    torch.cuda.synchronize()
    want_mul = [o.ckks_multiply(ct1[b], ct2[b], depth) for b in range(batch)]
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], want_mul[b]), "multiply"
    ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
    c.ckks_relinearize_inplace(out, 3 * l * n, dkey, depth, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    want_rel = [o.ckks_relinearize(want_mul[b].copy(), key, depth) for b in range(batch)]
    for b in range(batch):
        assert np.array_equal(got[b][:2 * l * n], want_rel[b][:2 * l * n]), "relinearize"
    if l >= 2:
        ws2 = c.workspace(hg.OP_CKKS_RESCALE, depth, batch)
        c.ckks_rescale_inplace(out, 3 * l * n, depth, batch, ws2)
        torch.cuda.synchronize()
        got = hg.to_host(out).reshape(batch, -1)
        for b in range(batch):
            w = o.ckks_rescale(want_rel[b][:2 * l * n].copy(), depth)
            assert np.array_equal(got[b][:2 * (l - 1) * n], w[:2 * (l - 1) * n]), "rescale"


@pytest.mark.parametrize("depth", [0, 1])
def test_ckks_keyswitch_mixed_widths_extreme_values(hg, oracle, torch, depth):
    """Key switch over a chain that mixes FP64 moduli (50/36/45/49 bits) with integer ones
    (60/55 bits): wide digits into narrow FP64 targets and vice versa, with the tensor input at
    its extremes (every residue q-1, then 0/q-1 patterns) and a key of all q-1."""
    n = 4096
    bits = [60, 50, 36, 45, 55, 49]
    c, o, primes = _ckks_pair(hg, oracle, n, bits, [60], sec=hg.SEC_NONE)
    Q, Qp = len(bits), len(bits) + 1
    l = Q - depth
    key = np.concatenate([np.full(n, primes[j] - 1, dtype=np.uint64) for _ in range(Q) for _c in range(2)
                          for j in range(Qp)])
    cts = []
    full = np.concatenate([np.full(n, primes[j] - 1, dtype=np.uint64) for _p in range(3) for j in range(l)])
    cts.append(full)
    pat = full.copy().reshape(3 * l, n); pat[:, ::3] = 0
    cts.append(pat.reshape(-1))
    cts.append(synth_ct(primes, range(l), 3, n, 77))
    batch = len(cts)
    d = hg.to_device(np.concatenate(cts))
    ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
    c.ckks_relinearize_inplace(d, 3 * l * n, hg.to_device(key), depth, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(d).reshape(batch, -1)
    for b in range(batch):
        want = o.ckks_relinearize(cts[b].copy(), key, depth)
        assert np.array_equal(got[b][:2 * l * n], want[:2 * l * n]), f"ciphertext {b}"


@pytest.mark.parametrize("depth", [0, 2])
def test_ckks_apply_galois(hg, oracle, torch, depth):
    n = 8192
    c, o, primes = _ckks_pair(hg, oracle, n, [40, 35, 35, 35], [40])
    Q, Qp = 4, 5
    l = Q - depth
    batch = 2
    gk = synth_key(primes, Q, Qp, n, 9)
    for steps in (1, -3):
        g = hg.steps_to_galois_elt(steps, n, 5)
        assert g == oracle.lib().o_steps_to_galois_elt(steps, n, 5)
        cts = [synth_ct(primes, range(l), 2, n, 5 + b) for b in range(batch)]
        d = hg.to_device(np.concatenate(cts))
        out = torch.empty_like(d)
        ws = c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
        c.ckks_apply_galois(d, 2 * l * n, out, 2 * l * n, hg.to_device(gk), g, depth, batch, ws)
        torch.cuda.synchronize()
        got = hg.to_host(out).reshape(batch, -1)
        for b in range(batch):
            assert np.array_equal(got[b], o.ckks_apply_galois(cts[b], gk, g, depth))


def test_bfv_multiply_relin_rotate(hg, oracle, torch):
    """Config C1 shapes on the GPU: BFV N=2^12 default chain, t=1032193."""
    n, t = 4096, 1032193
    c, o, primes = _bfv_pair(hg, oracle, n, t)
    Q, Qp = 2, 3
    batch = 3
    key = synth_key(primes, Q, Qp, n, 3)
    ct1 = [synth_ct(primes, range(Q), 2, n, 1 + 10 * b) for b in range(batch)]
    ct2 = [synth_ct(primes, range(Q), 2, n, 2 + 10 * b) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * Q * n, dtype=torch.int64, device="cuda")
    ws = c.workspace(hg.OP_BFV_MULTIPLY, 0, batch)
    c.bfv_multiply(d1, 2 * Q * n, d2, 2 * Q * n, out, 3 * Q * n, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    want_mul = [o.bfv_multiply(ct1[b], ct2[b]) for b in range(batch)]
    for b in range(batch):
        assert np.array_equal(got[b], want_mul[b]), "bfv multiply"
    ws = c.workspace(hg.OP_BFV_RELIN, 0, batch)
    c.bfv_relinearize_inplace(out, 3 * Q * n, hg.to_device(key), batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        w = o.bfv_relinearize(want_mul[b].copy(), key)
        assert np.array_equal(got[b][:2 * Q * n], w[:2 * Q * n]), "bfv relinearize"
    g = hg.steps_to_galois_elt(1, n, 3)
    rot = torch.empty(batch * 2 * Q * n, dtype=torch.int64, device="cuda")
    ws = c.workspace(hg.OP_BFV_GALOIS, 0, batch)
    c.bfv_apply_galois(d1, 2 * Q * n, rot, 2 * Q * n, hg.to_device(key), g, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(rot).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], o.bfv_apply_galois(ct1[b], key, g)), "bfv rotate"


def test_c3_bfv_rotate_batch64_full_size(hg, oracle, torch):
    """Config C3 at full size: BFV N=2^15, default chain (Q=14, P=1), rotate_rows
    by one step (Galois element 3, key-switch method I), batch 64; a sample of the
    batch is compared bit-for-bit with the oracle, the rest through the
    batch-consistency property (identical inputs -> identical outputs)."""
    n, t = 32768, 786433
    c, o, primes = _bfv_pair(hg, oracle, n, t)
    Q, Qp = c.Q_size, c.Q_prime_size
    assert (Q, Qp) == (14, 15)
    batch, uniq = 64, 4
    key = synth_key(primes, Q, Qp, n, 100)
    cts = [synth_ct(primes, range(Q), 2, n, 1 + b) for b in range(uniq)]
    per = 2 * Q * n
    d = torch.empty(batch * per, dtype=torch.int64, device="cuda")
    for b in range(batch):
        d[b * per:(b + 1) * per].copy_(torch.from_numpy(cts[b % uniq].view(np.int64)))
    out = torch.empty_like(d)
    g = hg.steps_to_galois_elt(1, n, 3)
    ws = c.workspace(hg.OP_BFV_GALOIS, 0, batch)
    c.bfv_apply_galois(d, per, out, per, hg.to_device(key), g, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, per)
    for b in range(uniq):
        assert np.array_equal(got[b], o.bfv_apply_galois(cts[b], key, g)), f"ciphertext {b}"
    for b in range(uniq, batch):
        assert np.array_equal(got[b], got[b % uniq]), f"batch item {b} differs from its twin"


@pytest.mark.parametrize("p_bits,reference_order", [([40, 40], False), ([40, 40], True), ([40, 41, 40], False),
                                                     ([60, 36, 45, 50], False)],
                         ids=["P2", "P2-reference-order", "P3", "P4-mixed-widths"])
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_ckks_method_II(hg, oracle, torch, depth, p_bits, reference_order, monkeypatch):
    """key-switching method II (P_size = 2, 3, 4): relinearize + rotate, leveled.  By default the multi-prime
    mod-down runs in the NTT domain (ops.cpp: ckks_moddown_multi); HEGPU_FUSED_MODDOWN=0 keeps the reference's
    order (INTT of every limb, k_moddown_extended in both its forms, NTT, addition)."""
    n = 8192
    if reference_order:
        monkeypatch.setenv("HEGPU_FUSED_MODDOWN", "0")  # read when the context is uploaded
    c, o, primes = _ckks_pair(hg, oracle, n, [40, 35, 35, 35, 35], p_bits, sec=hg.SEC_NONE)
    P = len(p_bits)
    Q, Qp = 5, 5 + P
    l = Q - depth
    d0 = -(-Q // P)
    batch = 2
    key = synth_key(primes, d0, Qp, n, 3)
    ct1 = [synth_ct(primes, range(l), 2, n, 1 + 10 * b) for b in range(batch)]
    ct2 = [synth_ct(primes, range(l), 2, n, 2 + 10 * b) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * l * n, dtype=torch.int64, device="cuda")
    c.ckks_multiply(d1, 2 * l * n, d2, 2 * l * n, out, 3 * l * n, depth, batch)
    ws = c.workspace(hg.OP_CKKS_RELIN, depth, batch)
    c.ckks_relinearize_inplace(out, 3 * l * n, hg.to_device(key), depth, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        w = o.ckks_multiply(ct1[b], ct2[b], depth)
        o.ckks_relinearize_II(w, key, depth)
        assert np.array_equal(got[b][:2 * l * n], w[:2 * l * n]), "method II relinearize"
    g = hg.steps_to_galois_elt(1, n, 5)
    rot = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
    ws = c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
    c.ckks_apply_galois(d1, 2 * l * n, rot, 2 * l * n, hg.to_device(key), g, depth, batch, ws)
    torch.cuda.synchronize()
    got = hg.to_host(rot).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], o.ckks_apply_galois_II(ct1[b], key, g, depth)), "method II rotate"


@pytest.mark.parametrize("shape", [(4096, [36, 36, 36], [37, 37], 1), (4096, [36, 36, 36], [37, 37], 0),
                                   (16384, [50, 59, 45, 50, 50], [59, 50, 60], 1), (32768, [58] * 6, [59, 59], 1)],
                         ids=["n12_fused", "n12_reference_order", "n14_three_special_primes", "n15_two_passes"])
def test_bfv_method_II(hg, oracle, torch, shape):
    """BFV key switching with several special primes (relinearize_external_product_method2_inplace / apply_galois
    method II, bfv/operator.cu:585-672, 866-973).  fused_moddown = 1: the mod-down by the special primes is the epilogue
    of the inverse transform of the Q limbs (NttInvEpilogue::u; single pass and two passes, FP64 and integer moduli);
    = 0: the reference's order with divide_round_lastq_extended / _permute kernels of their own."""
    n, log_q, log_p, fused = shape
    t = 1032193
    from helpers import backend_switches
    with backend_switches(HEGPU_FUSED_MODDOWN=fused):
        c = hg.Context.from_bit_sizes(hg.BFV, n, log_q, log_p, plain_modulus=t, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    Q, Qp, batch = len(log_q), len(log_q) + len(log_p), 2
    o = oracle.OracleContext(oracle.BFV, c.n_power, primes, Q, len(log_p), t)
    c.upload()
    key = synth_key(primes, -(-Q // 2), Qp, n, 3)
    ct1 = [synth_ct(primes, range(Q), 2, n, 1 + 10 * b) for b in range(batch)]
    ct2 = [synth_ct(primes, range(Q), 2, n, 2 + 10 * b) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_multiply(d1, 2 * Q * n, d2, 2 * Q * n, out, 3 * Q * n, batch, c.workspace(hg.OP_BFV_MULTIPLY, 0, batch))
    c.bfv_relinearize_inplace(out, 3 * Q * n, hg.to_device(key), batch, c.workspace(hg.OP_BFV_RELIN, 0, batch))
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        w = o.bfv_multiply(ct1[b], ct2[b])
        o.bfv_relinearize_II(w, key)
        assert np.array_equal(got[b][:2 * Q * n], w[:2 * Q * n]), "bfv method II relinearize"
    g = hg.steps_to_galois_elt(2, n, 3)
    rot = torch.empty(batch * 2 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_apply_galois(d1, 2 * Q * n, rot, 2 * Q * n, hg.to_device(key), g, batch,
                       c.workspace(hg.OP_BFV_GALOIS, 0, batch))
    torch.cuda.synchronize()
    got = hg.to_host(rot).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], o.bfv_apply_galois_II(ct1[b], key, g)), "bfv method II rotate"


def test_cpp_class_layer(torch):
    """include/heongpu/heongpu.hpp (HEContext / Ciphertext / Relinkey / Galoiskey /
    HEArithmeticOperator over the C ABI): tests/cpp/test_api.cpp vs the oracle."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "heongpu_amd", "lib", "test_cpp_api")
    assert os.path.exists(exe), "build it with __graft_entry__.build() (make -C heongpu_amd/csrc cpptest)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert "PASSED" in r.stdout


@pytest.mark.parametrize("name", ["ckks", "bfv", "tfhe"])
def test_reference_benchmark_runs_unchanged(torch, name, tmp_path):
    """benchmark/benchmark_{ckks,bfv}.cpp of the reference, compiled unchanged against the class
    layer by __graft_entry__.build() (oracle/ref_build.py, where the reference tree is available),
    run to completion."""
    import os
    import subprocess
    from oracle import ref_build
    exe = ref_build.exe_path("ref_benchmark_" + name)
    if not os.path.exists(exe):
        pytest.skip("reference benchmark binary not built (oracle/_ref/: no reference tree at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, cwd=tmp_path)
    print(r.stdout[-2500:], r.stderr[-500:])
    assert r.returncode == 0
    if name == "tfhe":
        assert "[NAND] Avg Time" in r.stdout and "[MUX] Avg Time" in r.stdout
    else:
        assert r.stdout.count("Average multiplication timing") >= 4


# what each of the reference's example programs must print (from the expected-result comments in
# example/basic/*.cpp); values are matched without the column padding of display_matrix/vector
_EXAMPLE_EXPECT = {
    "1_basic_bfv": ["[1,144,529,961,64,...,64,64,64,64,64]", "[49,2916,36,10000,64,...,64,64,64,64,64]",
                    "[6,864,3174,5766,384,...,384,384,384,384,384]", "[294,17496,216,60000,384,...,384,384,384,384,384]"],
    "2_basic_ckks": [(100.0, 400.0, 900.0, 1600.0, 9.0, 9.0, 9.0, 9.0), (50.0, 200.0, 450.0, 800.0, 4.5, 4.5, 4.5, 4.5)],
    "3_basic_memorypool_config": ["Q_tiltasize:Q(60+30+30+30)+P(60)bits", "DeviceMemoryPool"],
    "4_switchkey_methods_bfv": ["Checkresult4:[10000,64,64,64,64,...,64,64,49,2916,36][961,64,64,64,64,...,64,64,1,144,529]"],
    "5_switchkey_methods_ckks": ["Checkcheck3:", (1600.0, 0.25, 9.0, 9.0, 9.0, 100.0, 400.0, 900.0)],
    "8_default_stream_usage": ["Done."],
    "9_multi_stream_usage_way1": ["Done."],
    "10_multi_stream_usage_way2": ["Done."],
    "13_bfv_serialization": ["[961,64,64,64,64,...,64,64,1,144,529][10000,64,64,64,64,...,64,64,49,2916,36]"],
    # scale 2^30: the third decimal depends on the encryption noise -> compared numerically below
    "14_ckks_serialization": [(1600.0, 0.25, 9.0, 9.0, 9.0, 100.0, 400.0, 900.0)],
    "15_basic_tfhe": None,
}


@pytest.mark.parametrize("name", sorted(_EXAMPLE_EXPECT))
def test_reference_example_runs_unchanged(torch, name, tmp_path):
    """example/basic/<name>.cpp of the reference, compiled UNCHANGED against the class layer by
    __graft_entry__.build() (oracle/ref_build.py, where the reference tree is available), must run and
    print the results its own comments announce."""
    import os
    import re
    import subprocess
    from oracle import ref_build
    exe = ref_build.exe_path("ref_example_" + name)
    if not os.path.exists(exe):
        pytest.skip("reference example binary not built (oracle/_ref/: no reference tree at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    print(r.stdout[-2500:], r.stderr[-500:])
    assert r.returncode == 0
    flat = re.sub(r"\s+", "", r.stdout)
    if name == "15_basic_tfhe":
        def bits(label):
            m = re.search(r"^" + re.escape(label) + r"\s*([01, ]+)$", r.stdout, re.M)
            assert m, label
            return [int(v) for v in re.findall(r"[01]", m.group(1))]
        a, b, c = bits("Input1:"), bits("Input2:"), bits("Input3(control input of MUX):")
        assert len(a) == len(b) == len(c) == 8
        assert bits("NAND (Decrypted):") == [1 - (x & y) for x, y in zip(a, b)]
        assert bits("AND (Decrypted):") == [x & y for x, y in zip(a, b)]
        assert bits("NOR (Decrypted):") == [1 - (x | y) for x, y in zip(a, b)]
        assert bits("OR (Decrypted):") == [x | y for x, y in zip(a, b)]
        assert bits("XNOR (Decrypted):") == [1 - (x ^ y) for x, y in zip(a, b)]
        assert bits("XOR (Decrypted):") == [x ^ y for x, y in zip(a, b)]
        assert bits("NOT input1 (Decrypted):") == [1 - x for x in a]
        assert bits("MUX (Decrypted):") == [x if s else y for x, y, s in zip(a, b, c)]
        return
    for want in _EXAMPLE_EXPECT[name]:
        if isinstance(want, tuple):   # a displayed vector of doubles, to 0.01
            rows = [[float(v) for v in re.findall(r"-?\d+\.\d+", m)] for m in re.findall(r"\[([^\]]*)\]", r.stdout)]
            assert any(len(row) == len(want) and all(abs(a - b) < 1e-2 for a, b in zip(row, want)) for row in rows), rows
        else:
            assert want in flat, want


_REFERENCE_TESTS = ["test_bfv_addition", "test_bfv_encoding", "test_bfv_encryption", "test_bfv_multiplication",
                    "test_bfv_relinearization", "test_bfv_rotation_method_1", "test_bfv_rotation_method_2",
                    "test_ckks_addition", "test_ckks_encoding", "test_ckks_encryption", "test_ckks_multiplication",
                    "test_ckks_relinearization", "test_ckks_rotation_method_1", "test_ckks_rotation_method_2",
                    "test_tfhe_gate_boot"]


@pytest.mark.parametrize("name", _REFERENCE_TESTS)
def test_reference_own_test_passes(torch, name, tmp_path):
    """test/<name>.cpp of the reference -- its own encrypt -> operate -> decrypt checks over all its
    parameter sets (N = 2^12 .. 2^16, up to 37 primes, key-switching methods I and II) -- compiled
    UNCHANGED against the class layer (GoogleTest's TEST/EXPECT_EQ come from tests/cpp/gtest/gtest.h)
    by __graft_entry__.build() (oracle/ref_build.py), must pass on this backend."""
    import os
    import subprocess
    from oracle import ref_build
    exe = ref_build.exe_path("ref_" + name)
    if not os.path.exists(exe):
        pytest.skip("reference test binary not built (oracle/_ref/: no reference tree at build time)")
    # Every program must pass on its FIRST run.  The one exception is a flaw of the reference's own
    # test: test_bfv_addition.cpp:55,154,254,354,456 expect `(m1 + m2 > t) ? m1 + m2 - t : m1 + m2`, i.e.
    # the value t instead of 0 in a slot where m1 + m2 == t -- about n/t per parameter set, 16 % per run
    # over its five sets (fresh std::random_device messages on every run; measured here: 14 of 60 runs,
    # always in that comparison).  Only that program is repeated, and only when every failing assertion of
    # the run is one of those `message_addition_result` comparisons.
    import re
    for attempt in range(4):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=1500, cwd=tmp_path)
        print(r.stdout[-3000:], r.stderr[-1000:])
        if r.returncode == 0 or name != "test_bfv_addition":
            break
        failing = re.findall(r"Failure\nExpected equality of these values:\n\s+(.*)", r.stdout)
        if not failing or any("message_addition_result" not in f for f in failing) or "unexpected exception" in r.stdout:
            break
    assert r.returncode == 0
    assert "[  FAILED  ]" not in r.stdout and r.stdout.count("[       OK ]") >= 1


def test_cpp_api_writes_inside_its_buffers(torch):
    """tests/cpp/test_api.cpp again with 64 KiB canaries around every device buffer of the class layer
    (HEGPU_POOL_GUARD): no kernel may write outside the buffer it was given."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "heongpu_amd", "lib", "test_cpp_api")
    if not os.path.exists(exe):
        pytest.skip("test_cpp_api not built")
    env = dict(os.environ, HEGPU_POOL_GUARD="65536")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1500, env=env)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0 and "PASSED" in r.stdout
    assert "MemoryPool guard" not in r.stderr


def test_operator_sequence_replays_from_a_hip_graph(hg, oracle, torch):
    """The operator entry points neither allocate nor synchronise (caller workspace, caller stream), so a
    fixed sequence is capturable: multiply -> relinearize -> rescale -> rotate recorded once into a hipGraph
    (torch.cuda.CUDAGraph) and replayed on new inputs gives the oracle's results bit for bit (config C2
    shapes; the reference's multi-stream manager, util/storagemanager.cuh, reimplemented on HIP streams)."""
    n = 16384
    c, o, primes = _ckks_pair(hg, oracle, n, [50] + [40] * 7, [50])
    Q, Qp = 8, 9
    key = synth_key(primes, Q, Qp, n, 3)
    gal = hg.steps_to_galois_elt(1, n, 5)
    gkey = synth_key(primes, Q, Qp, n, 4)
    dkey, dgkey = hg.to_device(key), hg.to_device(gkey)
    d1 = torch.empty(2 * Q * n, dtype=torch.int64, device="cuda")
    d2 = torch.empty_like(d1)
    out = torch.empty(3 * Q * n, dtype=torch.int64, device="cuda")
    rot = torch.empty(2 * (Q - 1) * n, dtype=torch.int64, device="cuda")
    ws_relin = c.workspace(hg.OP_CKKS_RELIN, 0, 1)
    ws_resc = c.workspace(hg.OP_CKKS_RESCALE, 0, 1)
    ws_gal = c.workspace(hg.OP_CKKS_GALOIS, 1, 1)

    def sequence():
        c.ckks_multiply(d1, 2 * Q * n, d2, 2 * Q * n, out, 3 * Q * n, 0, 1)
        c.ckks_relinearize_inplace(out, 3 * Q * n, dkey, 0, 1, ws_relin)
        c.ckks_rescale_inplace(out, 3 * Q * n, 0, 1, ws_resc)
        c.ckks_apply_galois(out, 2 * (Q - 1) * n, rot, 2 * (Q - 1) * n, dgkey, gal, 1, 1, ws_gal)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm up outside the capture (lazy module loading)
        d1.zero_(); d2.zero_()
        sequence()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence()
    for seed in (1, 5):
        ct1 = synth_ct(primes, range(Q), 2, n, seed)
        ct2 = synth_ct(primes, range(Q), 2, n, seed + 1)
        d1.copy_(hg.to_device(ct1)); d2.copy_(hg.to_device(ct2))
        graph.replay()
        torch.cuda.synchronize()
        w = o.ckks_multiply(ct1, ct2, 0)
        o.ckks_relinearize(w, key, 0)
        w = o.ckks_rescale(w[:2 * Q * n].copy(), 0)[:2 * (Q - 1) * n]
        assert np.array_equal(hg.to_host(out)[:2 * (Q - 1) * n], w), "graph replay: multiply+relinearize+rescale"
        assert np.array_equal(hg.to_host(rot), o.ckks_apply_galois(w, gkey, gal, 1)), "graph replay: rotate"


_FUZZ = int(os.environ.get("HEGPU_FUZZ", "0"))  # extra seeds for a longer one-off run


@pytest.mark.parametrize("seed", range(16 + _FUZZ))
def test_random_parameter_sets(hg, oracle, torch, seed):
    """Seeded random CKKS parameter sets -- degree, number of primes, prime widths on both sides of the
    FP64 / integer split (2^50) and of the lazy-butterfly split (2^57), key-switching method, depth,
    batch -- through multiply -> relinearize -> rescale -> rotate, bit for bit against the oracle."""
    g = np.random.default_rng(1000 + seed)
    n = int(g.choice([4096, 8192, 16384]))
    Q = int(g.integers(2, 9))
    P = 1 if seed % 3 else 2
    widths = [30, 36, 40, 45, 49, 50, 51, 53, 57, 58, 60]
    log_q = [int(g.choice(widths)) for _ in range(Q)]
    log_p = [max(log_q)] * P if P == 1 else [max(max(log_q), 45)] * P
    log_p = [min(60, b + (1 if P == 1 else 0)) for b in log_p]
    try:
        c, o, primes = _ckks_pair(hg, oracle, n, log_q, log_p, sec=hg.SEC_NONE)
    except hg.HEError as e:            # "P should be bigger than Q pairs" for some draws
        pytest.skip(str(e))
    Qp = Q + P
    depth = int(g.integers(0, max(1, Q - 1)))
    l = Q - depth
    batch = int(g.integers(1, 4))
    rg, ro = hg.Rng(seed), oracle.ORng(seed)
    sk, sk_o = c.generate_secret_key(rg), o.gen_secret_key(ro)
    rk, rk_o = c.generate_relin_key(rg, sk), o.gen_switch_key(ro, sk_o, 0)
    gal = hg.steps_to_galois_elt(int(g.integers(1, 9)), n, 5)
    gk, gk_o = c.generate_galois_key(rg, sk, gal), o.gen_switch_key(ro, sk_o, gal)
    assert np.array_equal(hg.to_host(rk), rk_o) and np.array_equal(hg.to_host(gk), gk_o)
    ct1 = [synth_ct(primes, range(l), 2, n, 1 + 10 * b + seed) for b in range(batch)]
    ct2 = [synth_ct(primes, range(l), 2, n, 2 + 10 * b + seed) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * l * n, dtype=torch.int64, device="cuda")
    c.ckks_multiply(d1, 2 * l * n, d2, 2 * l * n, out, 3 * l * n, depth, batch)
    c.ckks_relinearize_inplace(out, 3 * l * n, rk, depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
    relin_o = o.ckks_relinearize if P == 1 else o.ckks_relinearize_II
    galois_o = o.ckks_apply_galois if P == 1 else o.ckks_apply_galois_II
    want = [relin_o(o.ckks_multiply(ct1[b], ct2[b], depth), rk_o, depth)[:2 * l * n] for b in range(batch)]
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b][:2 * l * n], want[b]), ("relinearize", n, log_q, log_p, depth, b)
    rot = torch.empty(batch * 2 * l * n, dtype=torch.int64, device="cuda")
    c.ckks_apply_galois(d1, 2 * l * n, rot, 2 * l * n, gk, gal, depth, batch, c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
    got = hg.to_host(rot).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], galois_o(ct1[b], gk_o, gal, depth)), ("rotate", n, log_q, log_p, depth, b)
    if l >= 2:
        c.ckks_rescale_inplace(out, 3 * l * n, depth, batch, c.workspace(hg.OP_CKKS_RESCALE, depth, batch))
        got = hg.to_host(out).reshape(batch, -1)
        for b in range(batch):
            w = o.ckks_rescale(want[b].copy(), depth)
            assert np.array_equal(got[b][:2 * (l - 1) * n], w[:2 * (l - 1) * n]), ("rescale", n, log_q, log_p, depth)


@pytest.mark.parametrize("seed", range(8 + _FUZZ))
def test_random_bfv_parameter_sets(hg, oracle, torch, seed):
    """Seeded random BFV parameter sets (degree, prime count and widths, plain modulus, key-switching method,
    batch) through multiply (BEHZ) -> relinearize -> rotate, bit for bit against the oracle."""
    g = np.random.default_rng(2000 + seed)
    n = int(g.choice([4096, 8192, 16384]))
    Q = int(g.integers(2, 7))
    P = 1 if seed % 2 else 2
    w = int(g.choice([36, 40, 45, 50, 54, 58, 59]))
    log_q = [w] * Q
    log_p = [min(60, w + 1)] * P
    t = int(g.choice([65537, 786433, 1032193]))
    try:
        c = hg.Context.from_bit_sizes(hg.BFV, n, log_q, log_p, plain_modulus=t, sec=hg.SEC_NONE)
    except hg.HEError as e:
        pytest.skip(str(e))
    primes = [int(x) for x in c.table("modulus")]
    o = oracle.OracleContext(oracle.BFV, c.n_power, primes, Q, P, t)
    c.upload()
    Qp = Q + P
    batch = int(g.integers(1, 4))
    rg, ro = hg.Rng(50 + seed), oracle.ORng(50 + seed)
    sk, sk_o = c.generate_secret_key(rg), o.gen_secret_key(ro)
    rk, rk_o = c.generate_relin_key(rg, sk), o.gen_switch_key(ro, sk_o, 0)
    gal = hg.steps_to_galois_elt(int(g.integers(1, 9)), n, 3)
    gk, gk_o = c.generate_galois_key(rg, sk, gal), o.gen_switch_key(ro, sk_o, gal)
    ct1 = [synth_ct(primes, range(Q), 2, n, 3 + 10 * b + seed) for b in range(batch)]
    ct2 = [synth_ct(primes, range(Q), 2, n, 4 + 10 * b + seed) for b in range(batch)]
    d1, d2 = hg.to_device(np.concatenate(ct1)), hg.to_device(np.concatenate(ct2))
    out = torch.empty(batch * 3 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_multiply(d1, 2 * Q * n, d2, 2 * Q * n, out, 3 * Q * n, batch, c.workspace(hg.OP_BFV_MULTIPLY, 0, batch))
    want = [o.bfv_multiply(ct1[b], ct2[b]) for b in range(batch)]
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], want[b]), ("multiply", n, log_q, log_p, t, b)
    c.bfv_relinearize_inplace(out, 3 * Q * n, rk, batch, c.workspace(hg.OP_BFV_RELIN, 0, batch))
    relin_o = o.bfv_relinearize if P == 1 else o.bfv_relinearize_II
    galois_o = o.bfv_apply_galois if P == 1 else o.bfv_apply_galois_II
    got = hg.to_host(out).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b][:2 * Q * n], relin_o(want[b].copy(), rk_o)[:2 * Q * n]), ("relinearize", n, log_q, log_p)
    rot = torch.empty(batch * 2 * Q * n, dtype=torch.int64, device="cuda")
    c.bfv_apply_galois(d1, 2 * Q * n, rot, 2 * Q * n, gk, gal, batch, c.workspace(hg.OP_BFV_GALOIS, 0, batch))
    got = hg.to_host(rot).reshape(batch, -1)
    for b in range(batch):
        assert np.array_equal(got[b], galois_o(ct1[b], gk_o, gal)), ("rotate", n, log_q, log_p)
