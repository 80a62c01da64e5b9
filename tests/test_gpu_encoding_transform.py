"""CoeffToSlot / SlotToCoeff (hegpu_ckks_conj_split, hegpu_ckks_conj_merge, hegpu_ckks_coeff_to_slot,
hegpu_ckks_slot_to_coeff), N = 4096.

  1. the two boundary passes against the composition of hegpu_addition (op 0 / 1) and hegpu_ckks_mult_i on the kept
     limbs, on synthetic residues of 60-bit moduli: exact;
  2. the sequence entries against the same chain of single entries (linear_transform, rescale_inplace, apply_galois,
     conj_split / conj_merge) on the same keys and inputs, key-switch methods I and II, two factors, batch 1 and 2:
     exact;
  3. semantics on the parameters of the reference's example ({50, 40 x 8} | {50}, scale 2^40, three pieces): after
     CoeffToSlot from depth 0, slot j of output 0 is a_bitrev(j) and of output 1 a_(n + bitrev(j)), imaginary parts
     ~ 0, under the reference tests' |a - b| < 1e-4 (encoding and key-switch error at scale 2^40 over three factors
     of at most 31 diagonals with entries of modulus <= 1 is of order N 2^-40 = 2^-28; a wrong order, twiddle or half
     gives order 1); after SlotToCoeff from there the decoded coefficients equal the decryption of the input under the
     example's own 5e-2 (the forward factors amplify by up to sqrt(n) .. n);
  4. refusals: HEGPU_E_INVALID and untouched outputs.
"""
import numpy as np
import pytest

from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
SLOTS = N // 2
SENT = 0x5555555555555555
EXAMPLE = ([50, 40, 40, 40, 40, 40, 40, 40, 40], [50])
SETS = {"method_I": EXAMPLE, "method_II": ([50, 40, 40, 40, 40, 40, 40, 40, 40], [50, 50])}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def bitrev(n):
    bits = n.bit_length() - 1
    j = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((j >> b) & 1) << (bits - 1 - b)
    return r


def elt(hg, shift):
    return hg.steps_to_galois_elt(shift, N, 5) if shift else 0


# ---------------------------------------------------------------- 1. the boundary passes
@pytest.fixture(scope="module")
def wide(hg, torch):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [60, 60, 60], [60], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    return c, primes


def _items(primes, l, batch, seed, pad):
    """batch ciphertexts [2][l][N] in a sentinel-filled buffer, `pad` words between the items"""
    words = 2 * l * N
    stride = words + pad
    cts = [synth_ct(primes, range(l), 2, N, seed + b).reshape(2, l, N) for b in range(batch)]
    buf = np.full(batch * stride, SENT, dtype=np.uint64)
    for b in range(batch):
        buf[b * stride:b * stride + words] = cts[b].reshape(-1)
    return cts, buf, stride


@pytest.mark.parametrize("l,drop", [(1, 0), (3, 0), (3, 1)])
def test_conj_split_and_merge_equal_the_composition(hg, torch, wide, l, drop):
    c, primes = wide
    Q, batch = c.Q_size, 2
    depth, out_depth, lo = Q - l, Q - l + drop, l - drop
    xs, xbuf, sx = _items(primes, l, batch, 10, N)
    ys, ybuf, sy = _items(primes, l, batch, 20, 3 * N)
    x, y = hg.to_device(xbuf), hg.to_device(ybuf)
    ow = 2 * lo * N
    so = ow + 2 * N
    out0 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    out1 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    merged = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    c.ckks_conj_split(x, sx, y, sy, out0, out1, so, depth, out_depth, batch)
    c.ckks_conj_merge(x, sx, y, sy, merged, so, depth, out_depth, batch)
    torch.cuda.synchronize()
    got0, got1, gotm = (hg.to_host(t).reshape(batch, so) for t in (out0, out1, merged))
    for b in range(batch):
        a = hg.to_device(np.ascontiguousarray(xs[b][:, :lo]).reshape(-1))  # the kept limbs of both parts
        k = hg.to_device(np.ascontiguousarray(ys[b][:, :lo]).reshape(-1))
        s, d = torch.empty_like(a), torch.empty_like(a)
        c.addition(a, k, s, lo, 2, 1, op=0)
        c.addition(a, k, d, lo, 2, 1, op=1)
        d = c.ckks_mult_i(d, lo, 2, divide=True)
        m = torch.empty_like(a)
        c.addition(a, c.ckks_mult_i(k, lo, 2, divide=False), m, lo, 2, 1, op=0)
        torch.cuda.synchronize()
        assert np.array_equal(got0[b, :ow], hg.to_host(s)), ("x + xc", l, drop, b)
        assert np.array_equal(got1[b, :ow], hg.to_host(d)), ("div_i(x - xc)", l, drop, b)
        assert np.array_equal(gotm[b, :ow], hg.to_host(m)), ("c0 + mult_i(c1)", l, drop, b)
        for g in (got0, got1, gotm):
            assert np.all(g[b, ow:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(x), xbuf) and np.array_equal(hg.to_host(y), ybuf), "the inputs are not written"


# ---------------------------------------------------------------- 2. sequences against the chain of single entries
def _synthetic_factors(hg, c, primes, inverse, pieces, first_depth, keys):
    """the plans of the real factorisation with synthetic diagonal residues; returns per factor the argument tuple of
    Context.linear_factors plus its plan"""
    out = []
    for f, g in enumerate(hg.encoding_transform_factors(N, inverse, pieces)):
        plan = hg.linear_transform_plan(g.offsets, SLOTS, stride=g.stride)
        l = c.Q_size - (first_depth + f)
        n_diag = len(g.offsets)
        diags = hg.to_device(np.concatenate([synth_ct(primes, range(l), 1, N, 1000 * (f + 1) + d) for d in range(n_diag)]))

        def key(shift):
            if not shift:
                return None
            if shift not in keys:
                keys[shift] = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 7 + shift))
            return keys[shift]
        out.append(((diags, n_diag, plan.index, [key(s) for s in plan.baby_shifts], [elt(hg, s) for s in plan.baby_shifts],
                     [key(s) for s in plan.giant_shifts], [elt(hg, s) for s in plan.giant_shifts]), plan))
    return out


def _chain(hg, torch, c, cur, cur_stride, factors, first_depth, batch, t_stride):
    """factor by factor: linear_transform into a fresh buffer, rescale_inplace there"""
    for f, (args, plan) in enumerate(factors):
        depth = first_depth + f
        dst = torch.full((batch * t_stride,), SENT, dtype=torch.int64, device="cuda")
        ws = torch.empty(c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, batch) // 8, dtype=torch.int64, device="cuda")
        diags, n_diag, index, bk, be, gk, ge = args
        c.ckks_linear_transform(cur, cur_stride, dst, t_stride, diags, n_diag, index, bk, be, gk, ge, depth, batch, ws)
        c.ckks_rescale_inplace(dst, t_stride, depth, batch, c.workspace(hg.OP_CKKS_RESCALE, depth, batch))
        cur, cur_stride = dst, t_stride
    return cur


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", list(SETS))
def test_sequences_equal_the_chain_of_single_entries(hg, torch, name, batch):
    log_q, log_p = SETS[name]
    c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    Q, P, keys = c.Q_size, 2, {}
    conj = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 5))
    # CoeffToSlot from depth 1
    depth = 1
    l = Q - depth
    _, cbuf, cs = _items(primes, l, batch, 300, N)
    ct = hg.to_device(cbuf)
    factors = _synthetic_factors(hg, c, primes, True, P, depth, keys)
    lo = l - P - 1
    ow = 2 * lo * N
    so = ow + N
    out0 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    out1 = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    args = [a for a, _ in factors]
    ws = torch.empty(c.encoding_transform_workspace_bytes(args, depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_coeff_to_slot(ct, cs, out0, out1, so, args, conj, depth, batch, ws)
    torch.cuda.synchronize()
    t_stride = 2 * l * N
    x = _chain(hg, torch, c, ct, cs, factors, depth, batch, t_stride)
    xc = torch.empty_like(x)
    c.ckks_apply_galois(x, t_stride, xc, t_stride, conj, 2 * N - 1, depth + P, batch, c.workspace(hg.OP_CKKS_GALOIS, depth + P, batch))
    w0, w1 = torch.empty(batch * ow, dtype=torch.int64, device="cuda"), torch.empty(batch * ow, dtype=torch.int64, device="cuda")
    c.ckks_conj_split(x, t_stride, xc, t_stride, w0, w1, ow, depth + P, depth + P + 1, batch)
    torch.cuda.synchronize()
    for got, want in ((out0, w0), (out1, w1)):
        g, w = hg.to_host(got).reshape(batch, so), hg.to_host(want).reshape(batch, ow)
        assert np.array_equal(g[:, :ow], w), (name, batch, "coeff_to_slot")
        assert np.all(g[:, ow:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"

    # SlotToCoeff from depth 2, on the two results
    depth = 2
    l = Q - depth
    _, abuf, sa = _items(primes, l, batch, 400, N)
    _, bbuf, sb = _items(primes, l, batch, 500, 2 * N)
    c0, c1 = hg.to_device(abuf), hg.to_device(bbuf)
    factors = _synthetic_factors(hg, c, primes, False, P, depth + 1, keys)
    assert max(plan.n2 for _, plan in factors) == 16, "six stages away from the last one: all sixteen giant steps"
    args = [a for a, _ in factors]
    room = 2 * (l - P) * N            # the last product is rescaled in the result buffer
    ow = 2 * (l - P - 1) * N
    so = room + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(args, depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_slot_to_coeff(c0, sa, c1, sb, out, so, args, depth, batch, ws)
    torch.cuda.synchronize()
    t_stride = 2 * (l - 1) * N
    merged = torch.empty(batch * t_stride, dtype=torch.int64, device="cuda")
    c.ckks_conj_merge(c0, sa, c1, sb, merged, t_stride, depth, depth + 1, batch)
    want = _chain(hg, torch, c, merged, t_stride, factors, depth + 1, batch, t_stride)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, t_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow]), (name, batch, "slot_to_coeff")
    assert np.all(g[:, room:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(c0), abuf) and np.array_equal(hg.to_host(c1), bbuf), "the inputs are not written"


# ---------------------------------------------------------------- 3. semantics
@pytest.fixture(scope="module")
def example(hg, torch):
    """context, keys and the encoded factors of both directions, three pieces: CoeffToSlot from depth 0, SlotToCoeff
    from depth 4"""
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *EXAMPLE, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    scale = 2.0 ** 40
    rng = hg.Rng(77)
    sk = c.generate_secret_key(rng)
    pk = c.generate_public_key(rng, sk)
    keys = {}

    def key(shift):
        if not shift:
            return None
        if shift not in keys:
            keys[shift] = c.generate_galois_key(rng, sk, elt(hg, shift))
        return keys[shift]

    def encoded(inverse, first_depth):
        out = []
        for f, g in enumerate(hg.encoding_transform_factors(N, inverse, 3)):
            plan = hg.linear_transform_plan(g.offsets, SLOTS, stride=g.stride)
            assert plan.n1 <= 8 and plan.n2 <= 8
            l = c.Q_size - (first_depth + f)
            order = np.argsort([k % SLOTS for k in g.offsets])  # the plan numbers the diagonals by k mod slots
            packed = torch.cat([c.ckks_encode_ex(1, torch.from_numpy(np.roll(g.diagonals[order[p]], -plan.pre_rotation[p])).cuda(),
                                                 scale)[:l * N] for p in range(len(order))])
            out.append((packed, len(order), plan.index, [key(s) for s in plan.baby_shifts], [elt(hg, s) for s in plan.baby_shifts],
                        [key(s) for s in plan.giant_shifts], [elt(hg, s) for s in plan.giant_shifts]))
        return out

    conj = c.generate_galois_key(rng, sk, 2 * N - 1)
    return c, primes, scale, rng, sk, pk, conj, encoded(True, 0), encoded(False, 5)


def _head_message():
    a = np.zeros(N)
    a[:8] = [1.00, -0.50, 0.25, -1.75, 2.50, -3.25, 0.125, -0.875]  # eight fixed values in [-4, 4]
    return a


@pytest.mark.parametrize("which", ["eight_values", "random_all_n"])
def test_coefficients_arrive_in_the_slots_and_return(hg, torch, example, which):
    c, primes, scale, rng, sk, pk, conj, ctos, stoc = example
    Q = c.Q_size
    a = _head_message() if which == "eight_values" else np.random.default_rng(3).uniform(-1, 1, N)
    ct = c.ckks_encrypt(rng, pk, c.ckks_encode_ex(2, torch.from_numpy(a).cuda(), scale))
    ow = 2 * (Q - 4) * N
    out0 = torch.empty(ow, dtype=torch.int64, device="cuda")
    out1 = torch.empty(ow, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(ctos, 0, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_coeff_to_slot(ct, 2 * Q * N, out0, out1, ow, ctos, conj, 0, 1, ws)
    sc = scale
    for f in range(3):  # every factor multiplies by its scale, the rescale divides by the modulus it drops
        sc = sc * scale / primes[Q - 1 - f]
    rev = bitrev(SLOTS)
    worst = 0.0
    for r, out in enumerate((out0, out1)):
        got = c.ckks_decode_ex(1, c.ckks_decrypt(out, sk, depth=4), sc, depth=4).cpu().numpy()
        worst = max(worst, np.abs(got - a[r * SLOTS + rev]).max())  # the imaginary part is part of the distance
    print(f"{which}: max |slot - coefficient| after coeff_to_slot = {worst:.3e} (criterion 1e-4)")
    assert worst < 1e-4

    room = 2 * (Q - 4 - 3) * N
    back = torch.empty(room, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.encoding_transform_workspace_bytes(stoc, 4, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_slot_to_coeff(out0, ow, out1, ow, back, room, stoc, 4, 1, ws)
    for f in range(3):
        sc = sc * scale / primes[Q - 6 - f]
    got = c.ckks_decode_ex(2, c.ckks_decrypt(back, sk, depth=8), sc, depth=8).cpu().numpy()
    ref = c.ckks_decode_ex(2, c.ckks_decrypt(ct, sk, depth=0), scale, depth=0).cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{which}: max |round trip - input| = {err:.3e} (criterion 5e-2)")
    assert err < 5e-2


# ---------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(hg, torch, example):
    c, primes, scale, rng, sk, pk, conj, ctos, stoc = example
    Q = c.Q_size
    words = 2 * Q * N
    ct = hg.to_device(synth_ct(primes, range(Q), 2, N, 1))
    other = hg.to_device(synth_ct(primes, range(Q), 2, N, 2))
    buf = torch.full((2 * words,), SENT, dtype=torch.int64, device="cuda")
    b0, b1 = buf[:words], buf[words:]
    ws = torch.empty(c.encoding_transform_workspace_bytes(ctos, 0, 1) // 8, dtype=torch.int64, device="cuda")

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote its result buffer"

    # out_depth out of range, batch < 1
    refused(lambda: c.ckks_conj_split(ct, words, other, words, b0, b1, words, 1, 0, 1))
    refused(lambda: c.ckks_conj_split(ct, words, other, words, b0, b1, words, 0, Q, 1))
    refused(lambda: c.ckks_conj_merge(ct, words, other, words, b0, words, 1, 0, 1))
    refused(lambda: c.ckks_conj_merge(ct, words, other, words, b0, words, 0, Q, 1))
    refused(lambda: c.ckks_conj_split(ct, words, other, words, b0, b1, words, 0, 0, 0))
    refused(lambda: c.ckks_conj_merge(ct, words, other, words, b0, words, 0, 0, 0))
    # a factor array of length 0; a depth that leaves fewer limbs than the factors (and the boundary) take
    refused(lambda: c.ckks_coeff_to_slot(ct, words, b0, b1, words, [], conj, 0, 1, ws))
    refused(lambda: c.ckks_slot_to_coeff(ct, words, other, words, b0, words, [], 0, 1, ws))
    refused(lambda: c.ckks_coeff_to_slot(ct, words, b0, b1, words, ctos, conj, Q - 4, 1, ws))
    refused(lambda: c.ckks_slot_to_coeff(ct, words, other, words, b0, words, stoc, Q - 4, 1, ws))
    # a short workspace
    refused(lambda: c.ckks_coeff_to_slot(ct, words, b0, b1, words, ctos, conj, 0, 1, ws[:ws.numel() - 1]))
    # overlapping buffers: an output on an input (sharing one word), the two outputs on each other
    both = torch.full((3 * words,), SENT, dtype=torch.int64, device="cuda")
    i0, i1 = both[:words], both[words:2 * words]
    clash = both[2 * words - 1:3 * words - 1]
    for fn in (lambda: c.ckks_conj_split(i0, words, i1, words, clash, b1, words, 0, 0, 1),
               lambda: c.ckks_conj_split(i0, words, i1, words, b0, i0, words, 0, 0, 1),
               lambda: c.ckks_conj_split(i0, words, i1, words, b0, b0, words, 0, 0, 1),
               lambda: c.ckks_conj_merge(i0, words, i1, words, clash, words, 0, 0, 1),
               lambda: c.ckks_coeff_to_slot(i0, words, b0, i0, words, ctos, conj, 0, 1, ws),
               lambda: c.ckks_coeff_to_slot(i0, words, b0, b0, words, ctos, conj, 0, 1, ws),
               lambda: c.ckks_slot_to_coeff(i0, words, i1, words, clash, words, stoc, 0, 1, ws)):
        refused(fn)
    torch.cuda.synchronize()
    assert bool((both == SENT).all())
    # valid arguments go through
    c.ckks_conj_split(ct, words, other, words, b0, b1, words, 0, 0, 1)
    torch.cuda.synchronize()
    assert not bool((b0 == SENT).all()) and not bool((b1 == SENT).all())
