"""GPU CKKS encoder / decoder where the kernels branch (heongpu_amd/csrc/encode.hip), against the oracle bit for bit
and against the independent reference of tests/embedding.py:

- every form of the special FFT (N = 2^12 .. 2^16: one LDS chunk with an odd / even stage count, one full 2^13 chunk,
  chunk + one or two outer stages) with message sizes inside and across the 2^13 boundary of the outer kernel;
- every instance of the CRT composition (LMAX = 8, 16, 32, 64) at the limb counts on both sides of each bound, on
  chosen integers (sign threshold, word boundaries, the low word of M) compared with exact integer arithmetic;
- scaled values beyond 2^63, 2^64 and up to just below 2^128, exact halves, -0.0 and subnormals;
- empty and null messages, through the C ABI and the Python API."""
import random
from fractions import Fraction

import numpy as np
import pytest

from embedding import compose_terms, crt_centered, embed, embed_bound, round_half_away

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_contexts = {}


def _pair(hg, oracle, n, log_q, log_p):
    key = (n, tuple(log_q), tuple(log_p))
    if key not in _contexts:
        c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
        c.upload()
        _contexts[key] = (c, o, primes)
    return _contexts[key]


def _same(a, b):
    """bit-identical doubles (complex arrays compared as their float64 pairs); a NaN matches any NaN, since the NaN a
    sum of +inf and -inf produces is not the same bit pattern on every processor"""
    a = np.ascontiguousarray(a).view(np.float64)
    b = np.ascontiguousarray(b).view(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return (a.shape == b.shape and np.array_equal(na, nb)
            and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def _dev(torch, msg, dtype):
    return torch.from_numpy(np.ascontiguousarray(msg, dtype=dtype)).cuda()


def _coefficients(o, l, plain):
    coeff = np.ascontiguousarray(plain, dtype=np.uint64).copy()
    o.ntt(coeff, l, l, inverse=True)
    return coeff


# ---- every form of the special FFT


@pytest.mark.parametrize("n_power", [12, 13, 14, 15, 16])
def test_slot_encode_decode_every_fft_form(hg, oracle, torch, n_power):
    n = 1 << n_power
    slots = n // 2
    c, o, primes = _pair(hg, oracle, n, [60, 40, 40], [60])
    g = np.random.default_rng(n_power)
    x = g.uniform(-100, 100, slots)
    z = g.uniform(-50, 50, slots) + 1j * g.uniform(-50, 50, slots)
    sizes = sorted({s for s in (0, 1, 3, 2**13 - 1, 2**13, 2**13 + 1, slots - 1, slots) if s <= slots})
    for size in sizes:
        plain = hg.to_host(c.ckks_encode(_dev(torch, x[:size], np.float64), SCALE))
        want = o.ckks_encode(x[:size], SCALE)
        assert np.array_equal(plain, want), f"real encode, size {size}"
        plain_z = hg.to_host(c.ckks_encode_ex(1, _dev(torch, z[:size], np.complex128), SCALE))
        want_z = o.ckks_encode_ex(1, z[:size], SCALE)
        assert np.array_equal(plain_z, want_z), f"complex encode, size {size}"
        for p in (want, want_z):
            dev = hg.to_device(p)
            assert _same(c.ckks_decode(dev, SCALE).cpu().numpy(), o.ckks_decode(p, SCALE)), f"real decode, size {size}"
            assert _same(c.ckks_decode_ex(1, dev, SCALE).cpu().numpy(), o.ckks_decode_ex(1, p, SCALE)), \
                f"complex decode, size {size}"
    # the GPU's plaintexts evaluated at the slot roots: message * scale (real: every slot; complex: a message ending
    # inside the outer kernel's first 2^13 block where there is one)
    for msg, mode in ((x, 0), (z[:min(2**13 + 1, slots - 1)], 1)):
        plain = hg.to_host(c.ckks_encode_ex(mode, _dev(torch, msg, np.complex128), SCALE) if mode else
                           c.ckks_encode(_dev(torch, msg, np.float64), SCALE))
        full = np.zeros(slots, dtype=np.complex128)
        full[:len(msg)] = msg
        got, conj = embed(crt_centered(_coefficients(o, 3, plain), primes[:3]), n, conjugates=True)
        bound = embed_bound(n, full, SCALE)
        assert np.all(np.abs(got - full * SCALE) <= bound), f"embedding of the mode-{mode} plaintext"
        assert np.all(np.abs(conj - np.conj(full) * SCALE) <= bound), f"conjugate slots of the mode-{mode} plaintext"


# ---- every width of the CRT composition

LONG_Q = [60] + [50] * 63      # 64 Q limbs: depth 64 - l leaves l of them
WIDTHS = [1, 2, 8, 9, 16, 17, 32, 33, 63, 64]


def _chosen_integers(primes):
    """the edge values of the composition for the modulus M = prod(primes), as integers in [0, M)"""
    M = 1
    for q in primes:
        M *= q
    m0, half = M & (2**64 - 1), (M + 1) // 2
    signed = [0, 1, -1, 2, -2, 2**52 - 1, -(2**52 - 1), m0 - 1, -(m0 - 1), (M - 1) // 2, half, half + 1, half - 1,
              M - 1]
    return M, [v % M for v in signed]


def _wide(M, count, rng):
    """random signed values of random bit length below M / 2 and 2^1000: every word count, finite decoded doubles"""
    top = min(M.bit_length() - 2, 1000)
    out = []
    for _ in range(count):
        v = rng.getrandbits(rng.randint(1, top))
        out.append(v if rng.random() < 0.5 else M - v)
    return out


def _plaintext(o, primes, values):
    l = len(primes)
    coeff = np.array([[v % q for v in values] for q in primes], dtype=np.uint64).reshape(-1)
    o.ntt(coeff, l, l)
    return coeff


def _overflowing(values, primes):
    """how many of the canonical values have a centred magnitude of 2^1000 or more: their terms (a borrow can reach one
    word above the value's top word) may exceed the double range, and the decoder's sum is not finite"""
    M = 1
    for q in primes:
        M *= q
    return sum(1 for v in values if min(v, M - v) >= 2**1000)


def _check_coeff_decode(got, values, primes, scale, positions, power_of_two):
    M = 1
    for q in primes:
        M *= q
    half, m0, l = (M + 1) // 2, M & (2**64 - 1), len(primes)
    checked = 0
    for i in positions:
        x = values[i] if values[i] < half else values[i] - M
        if abs(x) >= 2**1000:
            continue  # see _overflowing: the oracle comparison covers these
        terms = compose_terms(x, primes, scale)
        exact = Fraction(x) / Fraction(scale)
        r = float(got[i])
        assert np.isfinite(r), (l, i, x)
        if power_of_two and (0 <= x < 2**53 or -m0 < x < 0):
            assert r == float(exact), (l, i, x, r)  # one term, correctly rounded
        else:
            bound = (l + 2) * Fraction(2) ** -53 * sum(abs(t) for t in terms)
            assert abs(Fraction(r) - exact) <= bound, (l, i, x, r, float(exact))
        checked += 1
    return checked


def _decode_all_modes(hg, c, o, plain, depth, scale, modes=(0, 1, 2)):
    dev = hg.to_device(plain)
    out = {}
    for mode in modes:
        got = c.ckks_decode(dev, scale, depth) if mode == 0 else c.ckks_decode_ex(mode, dev, scale, depth)
        got = got.cpu().numpy()
        want = o.ckks_decode(plain, scale, depth) if mode == 0 else o.ckks_decode_ex(mode, plain, scale, depth)
        assert _same(got, want), f"mode {mode} decode at depth {depth}"
        out[mode] = got
    return out


@pytest.mark.parametrize("l", WIDTHS)
def test_decode_every_composition_width(hg, oracle, torch, l):
    n = 4096
    c, o, primes = _pair(hg, oracle, n, LONG_Q, [60])
    Q = len(LONG_Q)
    depth = Q - l
    qs = primes[:l]
    rng = random.Random(l)
    M, chosen = _chosen_integers(qs)
    # plaintext a: the chosen integers, then finite values of every width.  Near M / 2 they leave the double range
    # from l = 21 on, so the slot decodings, where one infinite coefficient turns every slot into NaN,
    # also run on plaintext f: the chosen integers that stay finite, and more of every width.
    a = chosen + _wide(M, n - len(chosen), rng)
    pa = _plaintext(o, qs, a)
    coeff_a = _decode_all_modes(hg, c, o, pa, depth, SCALE)[2]
    positions = list(range(len(chosen))) + rng.sample(range(len(chosen), n), 192)
    assert _check_coeff_decode(coeff_a, a, qs, SCALE, positions, True) == len(positions) - _overflowing(chosen, qs)
    f = [v for v in chosen if not _overflowing([v], qs)]
    f = f + _wide(M, n - len(f), rng)
    for slots in _decode_all_modes(hg, c, o, _plaintext(o, qs, f), depth, SCALE, (0, 1)).values():
        assert np.all(np.isfinite(slots.view(np.float64)))
    # plaintext b: uniform in [0, M) (mostly beyond the double range from l = 21 on: the oracle still decides)
    b = [rng.randrange(M) for _ in range(n)]
    coeff_b = _decode_all_modes(hg, c, o, _plaintext(o, qs, b), depth, SCALE)[2]
    _check_coeff_decode(coeff_b, b, qs, SCALE, rng.sample(range(n), 64), True)
    # a scale that is no power of two: within the bound only
    scale = SCALE * 1.37
    coeff_s = _decode_all_modes(hg, c, o, pa, depth, scale, (2,))[2]
    assert _check_coeff_decode(coeff_s, a, qs, scale, positions, False) == len(positions) - _overflowing(chosen, qs)


def test_decode_width_33_at_n_2_16(hg, oracle, torch):
    """the reference's large parameter set {60, 50 x 32} | {60}, at depth 0 (LMAX 64) and depth 1 (LMAX 32)"""
    n = 65536
    c, o, primes = _pair(hg, oracle, n, [60] + [50] * 32, [60])
    rng = random.Random(33)
    for depth in (0, 1):
        qs = primes[:33 - depth]
        M, chosen = _chosen_integers(qs)
        a = chosen + _wide(M, n - len(chosen), rng)
        coeff = _decode_all_modes(hg, c, o, _plaintext(o, qs, a), depth, SCALE)[2]
        positions = list(range(len(chosen))) + rng.sample(range(len(chosen), n), 128)
        assert _check_coeff_decode(coeff, a, qs, SCALE, positions, True) == len(positions) - _overflowing(chosen, qs)


def test_decode_rejects_65_limbs(hg, torch):
    c = hg.Context.from_bit_sizes(hg.CKKS, 4096, [60] + [50] * 64, [60], sec=hg.SEC_NONE)
    c.upload()
    zero = torch.zeros(65 * 4096, dtype=torch.int64, device="cuda")
    for mode in (0, 1, 2):
        with pytest.raises(hg.HEError):
            c.ckks_decode(zero, SCALE, 0) if mode == 0 else c.ckks_decode_ex(mode, zero, SCALE, 0)
        torch.cuda.synchronize()
    # one limb fewer composes
    got = c.ckks_decode_ex(2, zero[:64 * 4096], SCALE, 1).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), np.zeros(4096, dtype=np.uint64))


# ---- large and rounding-edge values

# (values >= 2^128 are out of scope: the conversion splits the rounded value into two 64-bit words, as the reference's
# 128-bit conversion does)
BIG = [2.0**63, 2.0**63 + 2.0**20, np.nextafter(2.0**64, 0), 2.0**64, 2.0**64 + 2.0**12, 1.2345 * 2.0**80, 2.0**100,
       1.9999 * 2.0**127, np.nextafter(2.0**128, 0)]
HALVES = [0.5, 1.5, 2.5, 3.5, 12345.5, 2.0**51 - 0.5, 0.49999999999999994]


def _edge_messages(scale):
    out = [b / scale for b in BIG] + [h / scale for h in HALVES]
    out = [m if m * scale < 2.0**128 else np.nextafter(m, 0) for m in out]  # (b / scale) * scale may round up to 2^128
    out = out + [-v for v in out]
    return out + [-0.0, 5e-324, 1.5e-310 / scale]


@pytest.mark.parametrize("scale", [SCALE, 1e12])
def test_large_and_rounding_edge_values(hg, oracle, torch, scale):
    n = 4096
    c, o, primes = _pair(hg, oracle, n, [60, 50, 50], [60])
    qs = primes[:3]
    edges = _edge_messages(scale)
    g = np.random.default_rng(7)
    msg = np.concatenate([np.array(edges), g.uniform(-1e3, 1e3, n - len(edges))])
    # coefficient encoding: residues = the oracle's, and the inverse NTT = round_half_away(m * scale) mod q_i exactly
    plain = hg.to_host(c.ckks_encode_ex(2, _dev(torch, msg, np.float64), scale))
    assert np.array_equal(plain, o.ckks_encode_ex(2, msg, scale)), "coefficient encode"
    coeff = _coefficients(o, 3, plain).reshape(3, n)
    for i, m in enumerate(edges):
        k = round_half_away(float(m) * scale)
        assert [int(coeff[j][i]) for j in range(3)] == [k % q for q in qs], (i, m)
    # scalar encoding: the constant polynomial, the same residue at every NTT point.  A negative double (-0.0 and
    # whatever rounds to it included) is reduced as q - (|k| mod q) with the reference's sub(q, 0) = q, so a multiple
    # of q, zero among them, is stored as q (the non-canonical q - 0)
    for m in edges:
        plain = hg.to_host(c.ckks_encode_ex(3, float(m), scale))
        assert np.array_equal(plain, o.ckks_encode_ex(3, [m], scale)), ("scalar encode", m)
        k = round_half_away(float(m) * scale)
        negative = np.signbit(float(m) * scale)
        want = np.concatenate([np.full(n, (q - abs(k) % q) if negative else k % q, dtype=np.uint64) for q in qs])
        assert np.array_equal(plain, want), ("scalar encode, exact", m)


# ---- empty and null messages


def _cabi(hg):
    return hg._lib.load()


@pytest.mark.parametrize("n_power", [12, 15, 16])
def test_empty_messages_encode_zero(hg, oracle, torch, n_power):
    """a NULL message of size 0 (what an empty tensor's data_ptr() is) encodes the zero polynomial, whatever the
    workspace holds -- N = 2^15 and 2^16: the message enters through the outer FFT kernel"""
    n = 1 << n_power
    c, o, primes = _pair(hg, oracle, n, [60, 40, 40], [60])
    lib, st = _cabi(hg), torch.cuda.current_stream().cuda_stream
    Q = 3
    zero = o.ckks_encode(np.zeros(0), SCALE)
    assert not zero.any()
    ws = c.workspace(hg.OP_CKKS_ENCODE, 0, 1)
    wbytes = ws.numel() * ws.element_size()

    def fresh():
        ws.view(torch.float64).fill_(1.0)  # what a stale transform would read
        return torch.full((Q * n,), 12345, dtype=torch.int64, device="cuda")

    wrong = []  # every path is tried; the report names each one that did not give the zero plaintext

    def expect_zero(what, plain, want=zero):
        got = hg.to_host(plain)
        if not np.array_equal(got, want):
            wrong.append(f"{what}: {np.count_nonzero(got)} non-zero residues, first {int(got[0])}")

    for name in ("hegpu_ckks_encode", "hegpu_ckks_encode_complex"):
        plain = fresh()
        assert getattr(lib, name)(c._h, None, 0, SCALE, plain.data_ptr(), ws.data_ptr(), wbytes, st) == 0, name
        torch.cuda.synchronize()
        expect_zero(name, plain)
    plain = fresh()
    assert lib.hegpu_ckks_encode_coeff(c._h, None, 0, SCALE, plain.data_ptr(), st) == 0
    torch.cuda.synchronize()
    expect_zero("hegpu_ckks_encode_coeff", plain, o.ckks_encode_ex(2, np.zeros(0), SCALE))
    # the Python API hands a null data_ptr() for an empty tensor
    expect_zero("ckks_encode", c.ckks_encode(torch.empty(0, dtype=torch.float64, device="cuda"), SCALE))
    expect_zero("ckks_encode_ex(1)", c.ckks_encode_ex(1, torch.empty(0, dtype=torch.complex128, device="cuda"), SCALE))
    expect_zero("ckks_encode_ex(2)", c.ckks_encode_ex(2, torch.empty(0, dtype=torch.float64, device="cuda"), SCALE))
    # BFV batch encoder
    b = hg.Context.from_default(hg.BFV, n, 1, 786433)
    b.upload()
    bzero = np.zeros(n, dtype=np.uint64)
    bp = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    assert lib.hegpu_bfv_encode(b._h, None, 0, bp.data_ptr(), st) == 0
    torch.cuda.synchronize()
    expect_zero("hegpu_bfv_encode", bp, bzero)
    expect_zero("bfv_encode", b.bfv_encode(torch.empty(0, dtype=torch.int64, device="cuda")), bzero)
    assert not wrong, "empty message: " + "; ".join(wrong)


def test_null_message_with_size_is_rejected(hg, oracle, torch):
    n = 4096
    c, o, primes = _pair(hg, oracle, n, [60, 40, 40], [60])
    lib, st = _cabi(hg), torch.cuda.current_stream().cuda_stream
    ws = c.workspace(hg.OP_CKKS_ENCODE, 0, 1)
    plain = torch.full((3 * n,), 12345, dtype=torch.int64, device="cuda")
    for name in ("hegpu_ckks_encode", "hegpu_ckks_encode_complex"):
        rc = getattr(lib, name)(c._h, None, 5, SCALE, plain.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)
        assert rc == hg.E_INVALID, name
    assert lib.hegpu_ckks_encode_coeff(c._h, None, 1, SCALE, plain.data_ptr(), st) == hg.E_INVALID
    b = hg.Context.from_default(hg.BFV, n, 1, 786433)
    b.upload()
    assert lib.hegpu_bfv_encode(b._h, None, 2, plain.data_ptr(), st) == hg.E_INVALID
    torch.cuda.synchronize()
    assert (plain == 12345).all().item(), "nothing written"
