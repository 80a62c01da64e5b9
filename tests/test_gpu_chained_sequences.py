"""Chained giant steps through the sequence entries (hegpu_linear_factor.giant_parent), N = 4096.

  1. hegpu_ckks_coeff_to_slot / _slot_to_coeff with chained factors against the chain of single entries
     (linear_transform_chained, rescale_inplace, apply_galois, conj_split / conj_merge), two and three pieces: exact;
  2. one call each of hegpu_ckks_bootstrap and hegpu_ckks_slim_bootstrap with chained factors against their chains, built
     as tests/test_gpu_bootstrap.py and tests/test_gpu_slim_bootstrap.py build them: exact;
  3. under encryption, with Galois keys for the reduced set only: CoeffToSlot -> SlotToCoeff on the parameters of the
     reference's example under the example's own 5e-2, one regular refresh and one slim refresh at the shapes and under
     the criteria (1e-4) of their existing semantic tests.  Each also runs the direct mode on the same input and prints
     both errors; the figures are recorded in DESIGN.md 4.5a / b / f / g.  The chain changes neither the number of key
     switches nor the diagonals, only the order in which the rotations act, so the error is of the same order.
"""
import numpy as np
import pytest

import test_gpu_bootstrap as boot
import test_gpu_slim_bootstrap as slim
from helpers import synth_ct, synth_key
from test_gpu_encoding_transform import EXAMPLE, SETS, _items, elt

pytestmark = pytest.mark.gpu

N = 4096
SLOTS = N // 2
SENT = 0x5555555555555555


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def transforms(hg, torch, c, cur, cur_stride, factors, first_depth, batch):
    """factor by factor: the chained (or direct) linear transform into a fresh buffer, rescale_inplace there"""
    for f, args in enumerate(factors):
        depth = first_depth + f
        stride = 2 * (c.Q_size - depth) * N
        dst = torch.full((batch * stride,), SENT, dtype=torch.int64, device="cuda")
        diags, n_diag, index, bk, be, gk, ge = args[:7]
        ws = torch.empty(c.linear_transform_workspace_bytes(len(be), len(ge), depth, batch) // 8, dtype=torch.int64, device="cuda")
        c.ckks_linear_transform(cur, cur_stride, dst, stride, diags, n_diag, index, bk, be, gk, ge, depth, batch, ws,
                                giant_parent=args[7] if len(args) > 7 else None)
        c.ckks_rescale_inplace(dst, stride, depth, batch, c.workspace(hg.OP_CKKS_RESCALE, depth, batch))
        cur, cur_stride = dst, stride
    return cur, cur_stride


def synthetic_chained_factors(hg, c, primes, inverse, pieces, first_depth, keys):
    """the plans of the real factorisation, chained, with synthetic diagonal residues and keys"""
    def key(e):
        if e not in keys:
            keys[e] = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 7 + e % 1000))
        return keys[e]

    out = []
    for f, g in enumerate(hg.encoding_transform_factors(N, inverse, pieces)):
        plan = hg.linear_transform_plan(g.offsets, SLOTS, stride=g.stride)
        l = c.Q_size - (first_depth + f)
        n_diag = len(g.offsets)
        diags = hg.to_device(np.concatenate([synth_ct(primes, range(l), 1, N, 1000 * (f + 1) + d) for d in range(n_diag)]))
        lkeys, lelts, parent, links = hg.chained_giant_steps(plan.giant_shifts, N, key)
        assert len({s for s in links if s}) <= 2
        belts = [elt(hg, s) for s in plan.baby_shifts]
        out.append((diags, n_diag, plan.index, [key(e) if e else None for e in belts], belts, lkeys, lelts, parent))
    return out


# ---------------------------------------------------------------- 1. CoeffToSlot / SlotToCoeff
@pytest.mark.parametrize("pieces", [2, 3])
def test_sequences_with_chained_factors_equal_the_chain_of_single_entries(hg, torch, pieces):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *SETS["method_I"], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    Q, P, keys, batch = c.Q_size, pieces, {}, 2
    conj = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 5))
    # CoeffToSlot from depth 1
    depth = 1
    l = Q - depth
    _, cbuf, cs = _items(primes, l, batch, 300, N)
    ct = hg.to_device(cbuf)
    factors = synthetic_chained_factors(hg, c, primes, True, P, depth, keys)
    assert any(p != -1 for f in factors for p in f[7])
    ow = 2 * (l - P - 1) * N
    so = ow + N
    out0 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    out1 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    direct = [f[:7] for f in factors]
    need = c.encoding_transform_workspace_bytes(factors, depth, batch)
    assert need == c.encoding_transform_workspace_bytes(direct, depth, batch), "one workspace size for both modes"
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    c.ckks_coeff_to_slot(ct, cs, out0, out1, so, factors, conj, depth, batch, ws)
    torch.cuda.synchronize()
    x, xs = transforms(hg, torch, c, ct, cs, factors, depth, batch)
    xc = torch.empty_like(x)
    c.ckks_apply_galois(x, xs, xc, xs, conj, 2 * N - 1, depth + P, batch, c.workspace(hg.OP_CKKS_GALOIS, depth + P, batch))
    w0, w1 = torch.empty(batch * ow, dtype=torch.int64, device="cuda"), torch.empty(batch * ow, dtype=torch.int64, device="cuda")
    c.ckks_conj_split(x, xs, xc, xs, w0, w1, ow, depth + P, depth + P + 1, batch)
    torch.cuda.synchronize()
    for got, want in ((out0, w0), (out1, w1)):
        g, w = hg.to_host(got).reshape(batch, so), hg.to_host(want).reshape(batch, ow)
        assert np.array_equal(g[:, :ow], w), (pieces, "coeff_to_slot")
        assert np.all(g[:, ow:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"

    # SlotToCoeff from depth 2
    depth = 2
    l = Q - depth
    _, abuf, sa = _items(primes, l, batch, 400, N)
    _, bbuf, sb = _items(primes, l, batch, 500, 2 * N)
    c0, c1 = hg.to_device(abuf), hg.to_device(bbuf)
    factors = synthetic_chained_factors(hg, c, primes, False, P, depth + 1, keys)
    room = 2 * (l - P) * N  # the last product is rescaled in the result buffer
    ow = 2 * (l - P - 1) * N
    so = room + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(factors, depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_slot_to_coeff(c0, sa, c1, sb, out, so, factors, depth, batch, ws)
    torch.cuda.synchronize()
    t_stride = 2 * (l - 1) * N
    merged = torch.empty(batch * t_stride, dtype=torch.int64, device="cuda")
    c.ckks_conj_merge(c0, sa, c1, sb, merged, t_stride, depth, depth + 1, batch)
    want, ws_stride = transforms(hg, torch, c, merged, t_stride, factors, depth + 1, batch)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, ws_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow]), (pieces, "slot_to_coeff")
    assert np.all(g[:, room:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(c0), abuf) and np.array_equal(hg.to_host(c1), bbuf), "the inputs are not written"


# ---------------------------------------------------------------- 2. the two refreshes on synthetic operands
def synthetic_refresh(hg, module, make_plan, seed0):
    c, primes = module.make_context(hg, "A")
    key = lambda seed: hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, seed))  # noqa: E731
    pool = [key(11), key(12), key(13)]
    keys = {k: key(20 + i) for i, k in enumerate(("conj", "relin", "d2s", "s2d"))}
    plan = make_plan(c, primes)
    seed = [0]

    def encode(values, scale, limbs):  # residues in place of an encoded diagonal
        seed[0] += 1
        return hg.to_device(synth_ct(primes, range(limbs), 1, N, seed0 + seed[0]))
    cts, stc, elts = c.bootstrap_factors(plan, lambda e: pool[e % 3], encode, chained=True)
    assert all(len(f) == 8 for f in cts + stc) and any(p != -1 for f in cts + stc for p in f[7])
    return c, primes, plan, cts, stc, keys


def test_bootstrap_with_chained_factors_equals_its_chain(hg, torch):
    c, primes, plan, cts, stc, keys = synthetic_refresh(
        hg, boot, lambda c, primes: hg.bootstrap_plan(primes[:c.Q_size], boot.DELTA, c.Q_size - 1, K=boot.K), 5000)
    batch = 2
    cs = 2 * N + N
    cbuf = np.full(batch * cs, SENT, dtype=np.uint64)
    for b in range(batch):
        cbuf[b * cs:b * cs + 2 * N] = synth_ct(primes, [0], 2, N, 900 + b)
    ct = hg.to_device(cbuf)
    ow, room = 2 * (plan.out_level + 1) * N, 2 * (plan.out_level + 2) * N
    so = room + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    need = c.bootstrap_workspace_bytes(plan, cts, stc, True, batch)
    assert need == c.bootstrap_workspace_bytes(plan, [f[:7] for f in cts], [f[:7] for f in stc], True, batch)
    ws = torch.full((need // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    c.ckks_bootstrap(ct, cs, out, so, plan, cts, stc, keys["conj"], keys["relin"], batch, ws[:need // 8],
                     swk_dense_to_sparse=keys["d2s"], swk_sparse_to_dense=keys["s2d"])
    torch.cuda.synchronize()
    want, ws_stride, _, _ = boot.chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, cs, batch, True)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, ws_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow])
    assert np.all(g[:, room:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"
    assert int(hg.to_host(ws[need // 8:])[0]) == SENT, "the word behind the workspace is intact"


def slim_chain(hg, torch, c, plan, cts, stc, keys, ct, cs, batch):
    """the slim refresh entry by entry (tests/test_gpu_slim_bootstrap.py::chain_of_single_entries, one input)"""
    Q = c.Q_size
    new = lambda words: torch.full((words,), SENT, dtype=torch.int64, device="cuda")  # noqa: E731
    cur, stride = transforms(hg, torch, c, ct, cs, stc, Q - 1 - plan.in_level, batch)
    raise_depth = Q - 1 - plan.cts_level
    rs = 2 * (plan.cts_level + 1) * N
    raised = new(batch * rs)
    c.ckks_mod_raise(cur, stride, raised, rs, raise_depth, batch, c.workspace(hg.OP_CKKS_MOD_RAISE, raise_depth, batch))
    cur, stride = transforms(hg, torch, c, raised, rs, cts, raise_depth, batch)
    d = raise_depth + plan.cts_pieces
    conj = new(batch * stride)
    c.ckks_apply_galois(cur, stride, conj, stride, keys["conj"], 2 * N - 1, d, batch, c.workspace(hg.OP_CKKS_GALOIS, d, batch))
    hs = 2 * (plan.eval_level + 1) * N
    real = new(batch * hs)
    c.ckks_conj_real(cur, stride, conj, stride, real, hs, d, d + 1, batch)
    es = 2 * plan.trig.out_limbs * N
    out = new(batch * es)
    depth = Q - 1 - plan.eval_level
    ws = torch.empty(max(c.poly_eval_workspace_bytes(plan.trig, depth, batch) // 8, 1), dtype=torch.int64, device="cuda")
    c.ckks_poly_eval(real, hs, out, es, plan.trig, keys["relin"], depth, batch, ws)
    return out, es


def test_slim_bootstrap_with_chained_factors_equals_its_chain(hg, torch):
    c, primes, plan, cts, stc, keys = synthetic_refresh(
        hg, slim, lambda c, primes: hg.slim_bootstrap_plan(primes[:c.Q_size], 2.0 ** 40, c.Q_size - 1, "slim"), 7000)
    batch = 2
    words = 2 * (plan.in_level + 1) * N
    cs = words + N
    cbuf = np.full(batch * cs, SENT, dtype=np.uint64)
    for b in range(batch):
        cbuf[b * cs:b * cs + words] = synth_ct(primes, range(plan.in_level + 1), 2, N, 900 + b)
    ct = hg.to_device(cbuf)
    ow = 2 * (plan.out_level + 1) * N
    assert plan.trig.out_limbs == plan.out_level + 1
    so = ow + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    need = c.slim_bootstrap_workspace_bytes(plan, cts, stc, batch)
    assert need == c.slim_bootstrap_workspace_bytes(plan, [f[:7] for f in cts], [f[:7] for f in stc], batch) > 0
    ws = torch.full((need // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    c.ckks_slim_bootstrap(ct, cs, out, so, plan, cts, stc, keys["conj"], keys["relin"], batch, ws[:need // 8])
    torch.cuda.synchronize()
    want, ws_stride = slim_chain(hg, torch, c, plan, cts, stc, keys, ct, cs, batch)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, ws_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow])
    assert np.all(g[:, ow:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"
    assert int(hg.to_host(ws[need // 8:])[0]) == SENT, "the word behind the workspace is intact"


# ---------------------------------------------------------------- 3. under encryption, reduced keys
class KeyRing:
    """Galois keys generated on demand, with a record of which elements were asked for"""

    def __init__(self, c, rng, sk):
        self.c, self.rng, self.sk, self.keys = c, rng, sk, {}

    def __call__(self, e):
        if e not in self.keys:
            self.keys[e] = self.c.generate_galois_key(self.rng, self.sk, e)
        return self.keys[e]


def test_round_trip_with_the_reduced_keys(hg, torch):
    """CoeffToSlot from depth 0, SlotToCoeff from depth 4 on {50, 40 x 8} | {50}, scale 2^40, three pieces"""
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *EXAMPLE, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    Q, scale = c.Q_size, 2.0 ** 40
    rng = hg.Rng(77)
    sk = c.generate_secret_key(rng)
    pk = c.generate_public_key(rng, sk)
    ring = KeyRing(c, rng, sk)

    def encoded(inverse, first_depth, chained):
        out = []
        for f, g in enumerate(hg.encoding_transform_factors(N, inverse, 3)):
            plan = hg.linear_transform_plan(g.offsets, SLOTS, stride=g.stride)
            l = Q - (first_depth + f)
            order = np.argsort([k % SLOTS for k in g.offsets])
            packed = torch.cat([c.ckks_encode_ex(1, torch.from_numpy(np.roll(g.diagonals[order[p]], -plan.pre_rotation[p])).cuda(),
                                                 scale)[:l * N] for p in range(len(order))])
            belts = [elt(hg, s) for s in plan.baby_shifts]
            bkeys = [ring(e) if e else None for e in belts]
            if chained:
                lkeys, lelts, parent, _ = hg.chained_giant_steps(plan.giant_shifts, N, ring)
                out.append((packed, len(order), plan.index, bkeys, belts, lkeys, lelts, parent))
            else:
                gelts = [elt(hg, s) for s in plan.giant_shifts]
                out.append((packed, len(order), plan.index, bkeys, belts, [ring(e) if e else None for e in gelts], gelts))
        return out

    modes = {"chained": (encoded(True, 0, True), encoded(False, 5, True))}
    reduced = set(ring.keys)
    modes["direct"] = (encoded(True, 0, False), encoded(False, 5, False))
    print(f"rotation keys: chained {len(reduced)}, direct {len(ring.keys)}")
    assert (len(reduced), len(ring.keys)) == (18, 29) and reduced < set(ring.keys)  # DESIGN.md 4.5a, N = 2^12, 3 + 3
    for f in modes["chained"][0] + modes["chained"][1]:  # the chained factors hold reduced keys only
        assert all(k is None or any(k is ring.keys[e] for e in reduced) for k in f[3] + f[5])
    conj = c.generate_galois_key(rng, sk, 2 * N - 1)
    a = np.random.default_rng(3).uniform(-1, 1, N)
    ct = c.ckks_encrypt(rng, pk, c.ckks_encode_ex(2, torch.from_numpy(a).cuda(), scale))
    ref = c.ckks_decode_ex(2, c.ckks_decrypt(ct, sk, depth=0), scale, depth=0).cpu().numpy()
    errs = {}
    for mode, (ctos, stoc) in modes.items():
        ow = 2 * (Q - 4) * N
        out0 = torch.empty(ow, dtype=torch.int64, device="cuda")
        out1 = torch.empty(ow, dtype=torch.int64, device="cuda")
        ws = torch.empty(c.encoding_transform_workspace_bytes(ctos, 0, 1) // 8, dtype=torch.int64, device="cuda")
        c.ckks_coeff_to_slot(ct, 2 * Q * N, out0, out1, ow, ctos, conj, 0, 1, ws)
        room = 2 * (Q - 4 - 3) * N
        back = torch.empty(room, dtype=torch.int64, device="cuda")
        ws = torch.empty(c.encoding_transform_workspace_bytes(stoc, 4, 1) // 8, dtype=torch.int64, device="cuda")
        c.ckks_slot_to_coeff(out0, ow, out1, ow, back, room, stoc, 4, 1, ws)
        sc = scale
        for f in range(3):
            sc = sc * scale / primes[Q - 1 - f]
        for f in range(3):
            sc = sc * scale / primes[Q - 6 - f]
        got = c.ckks_decode_ex(2, c.ckks_decrypt(back, sk, depth=8), sc, depth=8).cpu().numpy()
        errs[mode] = np.abs(got - ref).max()
    print(f"max |round trip - input|: chained {errs['chained']:.3e}, direct {errs['direct']:.3e} (criterion 5e-2)")
    assert errs["chained"] < 5e-2 and errs["direct"] < 5e-2


def test_regular_refresh_with_the_reduced_keys(hg, torch):
    """chain A, a secret of weight 32, no switch keys, all N coefficients: test_gpu_bootstrap.py::test_refreshed_coefficients"""
    c, primes = boot.make_context(hg, "A")
    plan = hg.bootstrap_plan(primes[:c.Q_size], boot.DELTA, c.Q_size - 1, K=boot.K)
    rng = hg.Rng(2026)
    sk = c.generate_secret_key(rng, 32)
    pk = c.generate_public_key(rng, sk)
    keys = {"relin": c.generate_relin_key(rng, sk)}
    ring = KeyRing(c, rng, sk)
    chained = c.bootstrap_factors(plan, ring, chained=True)
    reduced = set(ring.keys)
    assert sorted(reduced | {2 * N - 1}) == chained[2]
    direct = c.bootstrap_factors(plan, ring)
    keys["conj"] = ring(2 * N - 1)
    print(f"Galois keys, the conjugation included: chained {len(chained[2])}, direct {len(direct[2])}")
    assert (len(chained[2]), len(direct[2])) == (19, 30) and set(chained[2]) < set(direct[2])
    a = np.random.default_rng(5).uniform(-0.5, 0.5, N)
    ct = boot.exhausted(c, torch, rng, pk, c.ckks_encode_ex(2, torch.from_numpy(a).cuda(), boot.DELTA))
    _, _, raised, _ = boot.chain_of_single_entries(hg, torch, c, plan, chained[0], chained[1], keys, ct, 2 * N, 1, False)
    I, _ = boot.overflow_of_the_raise(hg, torch, c, primes, sk, raised, c.Q_size - 1 - plan.cts_level)
    assert np.abs(I).max() <= boot.K - 1, "an overflow of the raise outside the range EvalMod is built for"
    rho = primes[0] / (plan.k1 * boot.DELTA)
    depth = c.Q_size - 1 - plan.out_level
    errs = {}
    for mode, (cts, stc, _) in (("chained", chained), ("direct", direct)):
        out = boot.refresh(hg, torch, c, plan, keys, cts, stc, ct)
        got = c.ckks_decode_ex(2, c.ckks_decrypt(out, sk, depth=depth), plan.out_scale, depth=depth).cpu().numpy()
        errs[mode] = np.abs(got - boot.f_of(a, rho)).max()
    print(f"max |refreshed - f(a)| over {N} coefficients: chained {errs['chained']:.3e}, direct {errs['direct']:.3e} "
          "(criterion 1e-4)")
    assert errs["chained"] < 1e-4 and errs["direct"] < 1e-4


def test_slim_refresh_with_the_reduced_keys(hg, torch):
    """chain A, a secret of weight 32, all slots: test_gpu_slim_bootstrap.py::test_slim_refreshed_slots"""
    scale, rho = 2.0 ** 40, 256.0
    c, primes = slim.make_context(hg, "A")
    rng = hg.Rng(2027)
    sk = c.generate_secret_key(rng, 32)
    pk = c.generate_public_key(rng, sk)
    keys = {"relin": c.generate_relin_key(rng, sk)}
    ring = KeyRing(c, rng, sk)
    plan = hg.slim_bootstrap_plan(primes[:c.Q_size], scale, c.Q_size - 1, "slim")
    chained = c.slim_bootstrap_factors(plan, ring, chained=True)
    direct = c.slim_bootstrap_factors(plan, ring)
    keys["conj"] = ring(2 * N - 1)
    print(f"Galois keys, the conjugation included: chained {len(chained[2])}, direct {len(direct[2])}")
    assert (len(chained[2]), len(direct[2])) == (19, 30) and set(chained[2]) < set(direct[2])
    z = np.random.default_rng(5).uniform(-0.5, 0.5, SLOTS)
    ct = slim.encrypt_slots(c, torch, rng, pk, z, scale, plan.in_level + 1)
    slim.precondition(hg, torch, c, primes, sk, plan, direct[0], direct[1], keys, ct, None, "slim, direct factors")
    f = rho / (2 * np.pi) * np.sin(2 * np.pi * z / rho)
    errs = {mode: np.abs(slim.refresh(hg, torch, c, sk, plan, keys, cts, stc, ct) - f).max()
            for mode, (cts, stc, _) in (("chained", chained), ("direct", direct))}
    print(f"max |refreshed - f(z)| over {SLOTS} slots: chained {errs['chained']:.3e}, direct {errs['direct']:.3e} "
          "(criterion 1e-4)")
    assert errs["chained"] < 1e-4 and errs["direct"] < 1e-4
