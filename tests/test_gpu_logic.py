"""BFV / CKKS logic gates: hegpu_{ckks,bfv}_gate_combine (the one pass after the product) and hegpu_{ckks,bfv}_logic_gate
(the whole gate), DESIGN.md 4.5d.  The residue comparisons are exact: against Python integers, and against the chain of
entries that exist without the gates (multiply, relinearize, rescale, a host-side mod-drop copy, hegpu_addition,
hegpu_ckks_constant_op / hegpu_bfv_plain_addsub).  The truth tables go through encryption: a bit survives exactly when the
error of its slot is below 0.5.

The key-switch sets are those of test_gpu_poly_eval.py (method I: one special prime, method II: two)."""
import numpy as np
import pytest

from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
SETS = {"method_I": ([50, 30, 30, 30, 30, 30], [50]), "method_II": ([36, 36, 36, 36, 36, 36], [37, 37])}
BFV_SETS = {"method_I": ([36, 36, 36], [37]), "method_II": ([36, 36, 36], [37, 37])}
BFV_DEEP = ([54, 54, 54, 54], [55])  # the full adder multiplies three times in a row
T = 65537
SENTINEL = 0x5A5A5A5A5A5A5A5A
GATES = {"AND": (0, 0, 1), "OR": (0, 1, -1), "XOR": (0, 1, -2), "NAND": (1, 0, -1), "NOR": (1, -1, 1), "XNOR": (1, -1, 2),
         "NOT": (1, -1, 0)}
TABLE = {"AND": lambda x, y: x & y, "OR": lambda x, y: x | y, "XOR": lambda x, y: x ^ y, "NAND": lambda x, y: 1 - (x & y),
         "NOR": lambda x, y: 1 - (x | y), "XNOR": lambda x, y: 1 - (x ^ y)}
BINARY = [g for g in GATES if g != "NOT"]
NONE, CIPHER, PLAIN = 0, 1, 2
BIG_ONE = float(2 ** 80 + 12345 * 2 ** 30)  # exact in a double; beyond 64 bits


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_contexts = {}


def context(hg, scheme, log_q, log_p):
    key = (scheme, tuple(log_q), tuple(log_p))
    if key not in _contexts:
        c = hg.Context.from_bit_sizes(scheme, N, list(log_q), list(log_p), plain_modulus=T if scheme == hg.BFV else 0,
                                      sec=hg.SEC_NONE)
        c.upload()
        _contexts[key] = (c, [int(x) for x in c.table("modulus")])
    return _contexts[key]


def gate_id(hg, name):
    return getattr(hg, "LOGIC_" + name)


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def padded(hg, items, pad):
    """items: host arrays of equal length -> (device tensor with sentinel padding, stride, offset of item 0)"""
    words = len(items[0])
    stride = words + pad
    buf = np.full(pad + stride * len(items), SENTINEL, dtype=np.uint64)
    for b, it in enumerate(items):
        buf[pad + b * stride: pad + b * stride + words] = it
    return hg.to_device(buf), stride, pad


def assert_only_out_written(got, off, so, out_words, batch):
    mask = np.ones(len(got), dtype=bool)
    for b in range(batch):
        mask[off + b * so: off + b * so + out_words] = False
    assert np.all(got[mask] == SENTINEL), "a word outside out was written"


def model(name, a, b, p, one, q):
    """Python integers: c0 * one + c1 * (a + b) + c2 * p mod q; absent operands are None"""
    c0, c1, c2 = GATES[name]
    acc = np.zeros(N, dtype=object)
    if c0 and one is not None:
        acc = acc + one
    if c1:
        s = a.astype(object)
        if b is not None:
            s = s + b.astype(object)
        acc = acc + c1 * s
    if c2:
        acc = acc + c2 * p.astype(object)
    return np.array(acc % q, dtype=np.uint64)


def ckks_combine_case(hg, torch, limbs, scale_one, maximal, seed):
    """every gate with b as ciphertext, plaintext and none; a one level, b two levels above the result"""
    c, primes = context(hg, hg.CKKS, [60, 40, 40, 40, 40], [60])
    assert primes[0].bit_length() >= 60
    a_limbs, b_limbs, p_limbs, batch = limbs + 1, limbs + 2, limbs, 2

    def operand(L, parts, s):
        if maximal:
            return [np.concatenate([np.full(N, primes[j] - 1, dtype=np.uint64) for _ in range(parts) for j in range(L)])
                    for _ in range(batch)]
        return [synth_ct(primes, range(L), parts, N, s + i) for i in range(batch)]

    a, bc, bp, p = operand(a_limbs, 2, seed), operand(b_limbs, 2, seed + 10), operand(b_limbs, 1, seed + 20), operand(p_limbs, 2, seed + 30)
    da, sa, oa = padded(hg, a, 64)
    dbc, sbc, obc = padded(hg, bc, 66)
    dbp, sbp, obp = padded(hg, bp, 68)
    dp, sp, op = padded(hg, p, 70)
    out_words = 2 * limbs * N
    one_int = int(round(scale_one))
    for name in GATES:
        for kind in ([NONE] if name == "NOT" else [CIPHER, PLAIN]):
            out, so, off = padded(hg, [np.full(out_words, SENTINEL, dtype=np.uint64)] * batch, 128)
            b_dev, b_stride, b_host = {NONE: (None, 0, None), CIPHER: (dbc[obc:], sbc, bc), PLAIN: (dbp[obp:], sbp, bp)}[kind]
            c.ckks_gate_combine(gate_id(hg, name), da[oa:], sa, a_limbs, b_dev, kind, b_stride, b_limbs if kind else 0,
                                None if name == "NOT" else dp[op:], 0 if name == "NOT" else sp, 0 if name == "NOT" else p_limbs,
                                scale_one, out[off:], so, limbs, batch=batch)
            torch.cuda.synchronize()
            got = hg.to_host(out)
            for i in range(batch):
                res = got[off + i * so: off + i * so + out_words].reshape(2, limbs, N)
                for z in range(2):
                    for j in range(limbs):
                        q = primes[j]
                        bj = None
                        if kind == CIPHER:
                            bj = b_host[i].reshape(2, b_limbs, N)[z, j]
                        elif kind == PLAIN and z == 0:
                            bj = b_host[i].reshape(b_limbs, N)[j]
                        want = model(name, a[i].reshape(2, a_limbs, N)[z, j], bj, p[i].reshape(2, p_limbs, N)[z, j],
                                     one_int % q if z == 0 else None, q)
                        assert np.array_equal(res[z, j], want), (name, kind, limbs, i, z, j)
            assert_only_out_written(got, off, so, out_words, batch)


@pytest.mark.parametrize("scale_one", [2.0 ** 30, BIG_ONE])
@pytest.mark.parametrize("limbs", [1, 3])
def test_ckks_combine_against_python_integers(hg, torch, limbs, scale_one):
    """batch 2, padded item strides, unequal limb counts (a: limbs + 1, b: limbs + 2, p: limbs), sentinels around out"""
    ckks_combine_case(hg, torch, limbs, scale_one, False, 500 + limbs)


def test_ckks_combine_maximal(hg, torch):
    """every residue q - 1 on the chain [60, 40, 40, 40, 40]: the largest operands the modular additions can meet"""
    ckks_combine_case(hg, torch, 3, BIG_ONE, True, 0)


# ---------------------------------------------------------------------------------------------- the chain of single entries
def drop(t, batch, limbs_in, limbs, parts=2):
    """the first `limbs` limbs of every part of a contiguous batch [batch][parts][limbs_in][N]: always a copy (mod_drop)"""
    return t.view(batch, parts, limbs_in, N)[:, :, :limbs].clone().reshape(-1)


def bfv_plain_add(c, torch, ct, plain):
    out = torch.empty_like(ct)
    assert c._lib.hegpu_bfv_plain_addsub(c._h, ct.data_ptr(), plain.data_ptr(), out.data_ptr(), 0, stream(torch)) == 0
    return out


def chain_tail(c, hg, torch, bfv, name, a, b, kind, p, limbs, batch, scale_one):
    """The part of a gate after the product with entries that exist without the gates.  a, p and a ciphertext b: contiguous
    [batch][2][limbs][N]; a plaintext b: [batch][limbs][N] (CKKS) or [batch][N] (BFV)."""
    c0, c1, c2 = GATES[name]
    words = 2 * limbs * N
    r = None
    if c1:
        r = a.clone()
        if kind == CIPHER:
            c.addition(r, b, r, limbs, 2, batch)
        elif kind == PLAIN:
            for i in range(batch):
                if bfv:
                    r[i * words:(i + 1) * words] = bfv_plain_add(c, torch, r[i * words:(i + 1) * words].clone(), b[i * N:(i + 1) * N])
                else:  # a CKKS plaintext is added to part 0 with hegpu_addition
                    c.addition(r[i * words:], b[i * limbs * N:], r[i * words:], limbs, 1, 1)
        if c1 < 0:
            c.addition(r, r, r, limbs, 2, batch, op=2)
    if c2:
        pp = p.clone()
        if abs(c2) == 2:
            c.addition(pp, pp, pp, limbs, 2, batch)
        if r is None:
            r = pp
            if c2 < 0:
                c.addition(r, r, r, limbs, 2, batch, op=2)
        else:
            c.addition(r, pp, r, limbs, 2, batch, op=0 if c2 > 0 else 1)
    if c0:
        e0 = torch.zeros(N, dtype=torch.int64, device="cuda")
        e0[0] = 1
        for i in range(batch):
            if bfv:
                r[i * words:(i + 1) * words] = bfv_plain_add(c, torch, r[i * words:(i + 1) * words].clone(), e0)
            else:
                c.ckks_constant_op(0, r[i * words:], scale_one, limbs, 2, out=r[i * words:])
    return r


def bfv_scaled(m, j, primes, coeff_div, q_mod_t, threshold):
    """floor(Q / t) * m + fix mod q_j with Python integers"""
    return [(int(v) * coeff_div[j] + (int(v) * q_mod_t + threshold) // T) % primes[j] for v in m]


def test_bfv_combine_against_python_integers_and_the_plain_add(hg, torch):
    """Q_size 3, t = 65537, every gate, ciphertext and plaintext b, batch 2 with padded strides.  The constant one and the
    plaintext term are also compared, bit for bit, with hegpu_addition (negate) + hegpu_bfv_plain_addsub."""
    c, primes = context(hg, hg.BFV, *BFV_SETS["method_I"])
    Q, batch = 3, 2
    assert c.Q_size == Q
    cd = [int(x) for x in c.table("coeff_div_plain_modulus")]
    q_mod_t, thr = int(c.table("Q_mod_t")[0]), int(c.table("upper_threshold")[0])
    rng = np.random.default_rng(9)
    a = [synth_ct(primes, range(Q), 2, N, 700 + i) for i in range(batch)]
    bc = [synth_ct(primes, range(Q), 2, N, 710 + i) for i in range(batch)]
    bp = [rng.integers(0, T, N).astype(np.uint64) for _ in range(batch)]
    bp[0][:3] = [0, 1, T - 1]
    p = [synth_ct(primes, range(Q), 2, N, 720 + i) for i in range(batch)]
    da, sa, oa = padded(hg, a, 64)
    dbc, sbc, obc = padded(hg, bc, 66)
    dbp, sbp, obp = padded(hg, bp, 68)
    dp, sp, op = padded(hg, p, 70)
    words = 2 * Q * N
    ca, cbc, cbp, cp = (hg.to_device(np.concatenate(x)) for x in (a, bc, bp, p))
    one = np.zeros(N, dtype=np.uint64)
    for name in GATES:
        for kind in ([NONE] if name == "NOT" else [CIPHER, PLAIN]):
            out, so, off = padded(hg, [np.full(words, SENTINEL, dtype=np.uint64)] * batch, 128)
            b_dev, b_stride = {NONE: (None, 0), CIPHER: (dbc[obc:], sbc), PLAIN: (dbp[obp:], sbp)}[kind]
            c.bfv_gate_combine(gate_id(hg, name), da[oa:], sa, b_dev, kind, b_stride, None if name == "NOT" else dp[op:],
                               0 if name == "NOT" else sp, out[off:], so, batch=batch)
            want_chain = chain_tail(c, hg, torch, True, name, ca, {NONE: None, CIPHER: cbc, PLAIN: cbp}[kind], kind, cp, Q, batch, 0.0)
            torch.cuda.synchronize()
            got = hg.to_host(out)
            chain = hg.to_host(want_chain)
            for i in range(batch):
                res = got[off + i * so: off + i * so + words]
                assert np.array_equal(res, chain[i * words:(i + 1) * words]), (name, kind, i, "chain")
                res = res.reshape(2, Q, N)
                for z in range(2):
                    for j in range(Q):
                        bj = None
                        if kind == CIPHER:
                            bj = bc[i].reshape(2, Q, N)[z, j]
                        elif kind == PLAIN and z == 0:
                            bj = np.array(bfv_scaled(bp[i], j, primes, cd, q_mod_t, thr), dtype=np.uint64)
                        one[0] = bfv_scaled([1], j, primes, cd, q_mod_t, thr)[0]
                        want = model(name, a[i].reshape(2, Q, N)[z, j], bj, p[i].reshape(2, Q, N)[z, j],
                                     one.astype(object) if z == 0 else None, primes[j])
                        assert np.array_equal(res[z, j], want), (name, kind, i, z, j)
            assert_only_out_written(got, off, so, words, batch)
    # in place: out is a itself
    a2 = ca.clone()
    c.bfv_gate_combine(hg.LOGIC_XNOR, a2, words, cbc, CIPHER, words, cp, words, a2, words, batch=batch)
    want = chain_tail(c, hg, torch, True, "XNOR", ca, cbc, CIPHER, cp, Q, batch, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(a2, want)


# ---------------------------------------------------------------------------------------------- fused entry == composition
def ckks_compose(c, hg, torch, name, a, b, kind, key, depth, batch, scale_one):
    Q = c.Q_size
    l = Q - depth
    if name == "NOT":
        return chain_tail(c, hg, torch, False, name, a, None, NONE, None, l, batch, scale_one)
    if kind == CIPHER:
        prod = torch.empty(batch * 3 * l * N, dtype=torch.int64, device="cuda")
        stride = 3 * l * N
        c.ckks_multiply(a, 2 * l * N, b, 2 * l * N, prod, stride, depth, batch)
        c.ckks_relinearize_inplace(prod, stride, key, depth, batch, c.workspace(hg.OP_CKKS_RELIN, depth, batch))
    else:
        prod = torch.empty(batch * 2 * l * N, dtype=torch.int64, device="cuda")
        stride = 2 * l * N
        for i in range(batch):
            assert c._lib.hegpu_cipherplain_multiplication(c._h, a[i * stride:].data_ptr(), b[i * l * N:].data_ptr(),
                                                           prod[i * stride:].data_ptr(), l, stream(torch)) == 0
    c.ckks_rescale_inplace(prod, stride, depth, batch, c.workspace(hg.OP_CKKS_RESCALE, depth, batch))
    p = prod.view(batch, stride)[:, :2 * (l - 1) * N].contiguous().view(-1)
    b_low = drop(b, batch, l, l - 1) if kind == CIPHER else drop(b, batch, l, l - 1, parts=1)
    return chain_tail(c, hg, torch, False, name, drop(a, batch, l, l - 1), b_low, kind, p, l - 1, batch, scale_one)


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("kind", [CIPHER, PLAIN])
@pytest.mark.parametrize("name", list(SETS))
def test_ckks_logic_gate_equals_its_composition(hg, torch, name, kind, depth):
    c, primes = context(hg, hg.CKKS, *SETS[name])
    Q, Qp, batch = c.Q_size, c.Q_prime_size, 2
    l = Q - depth
    a = hg.to_device(np.concatenate([synth_ct(primes, range(l), 2, N, 40 + i) for i in range(batch)]))
    b = hg.to_device(np.concatenate([synth_ct(primes, range(l), 2 if kind == CIPHER else 1, N, 50 + i) for i in range(batch)]))
    key = hg.to_device(synth_key(primes, c.switch_key_digits(), Qp, N, 3))
    ws = c.workspace(hg.OP_CKKS_LOGIC_GATE, depth, batch)
    scale_one = float(primes[1])
    for gate in GATES:
        unary = gate == "NOT"
        out_limbs = l if unary else l - 1
        so = 2 * out_limbs * N + 32
        out = torch.full((batch * so,), SENTINEL, dtype=torch.int64, device="cuda")
        c.ckks_logic_gate(gate_id(hg, gate), a, 2 * l * N, None if unary else b, NONE if unary else kind,
                          0 if unary else b.numel() // batch, None if unary else key, scale_one, out, so, depth, batch,
                          None if unary else ws)
        want = ckks_compose(c, hg, torch, gate, a, b, kind, key, depth, batch, scale_one)
        torch.cuda.synchronize()
        assert torch.equal(out.view(batch, so)[:, :2 * out_limbs * N].contiguous().view(-1), want), (gate, name, kind, depth)
        assert bool((out.view(batch, so)[:, 2 * out_limbs * N:] == SENTINEL).all()), "written past the result"


@pytest.mark.parametrize("kind", [CIPHER, PLAIN])
@pytest.mark.parametrize("name", list(BFV_SETS))
def test_bfv_logic_gate_equals_its_composition(hg, torch, name, kind):
    c, primes = context(hg, hg.BFV, *BFV_SETS[name])
    Q, Qp, batch = c.Q_size, c.Q_prime_size, 2
    words = 2 * Q * N
    a = hg.to_device(np.concatenate([synth_ct(primes, range(Q), 2, N, 60 + i) for i in range(batch)]))
    if kind == CIPHER:
        b = hg.to_device(np.concatenate([synth_ct(primes, range(Q), 2, N, 70 + i) for i in range(batch)]))
    else:
        b = hg.to_device(np.random.default_rng(4).integers(0, T, batch * N).astype(np.uint64))
    key = hg.to_device(synth_key(primes, c.switch_key_digits(), Qp, N, 5))
    ws = c.workspace(hg.OP_BFV_LOGIC_GATE, 0, batch)
    # the product once, with the single entries
    if kind == CIPHER:
        prod = torch.empty(batch * 3 * Q * N, dtype=torch.int64, device="cuda")
        c.bfv_multiply(a, words, b, words, prod, 3 * Q * N, batch, c.workspace(hg.OP_BFV_MULTIPLY, 0, batch))
        c.bfv_relinearize_inplace(prod, 3 * Q * N, key, batch, c.workspace(hg.OP_BFV_RELIN, 0, batch))
        p = prod.view(batch, 3 * Q * N)[:, :words].contiguous().view(-1)
    else:
        p = torch.empty(batch * words, dtype=torch.int64, device="cuda")
        w1 = c.workspace(hg.OP_BFV_MULTIPLY_PLAIN, 0, 1)
        for i in range(batch):
            assert c._lib.hegpu_bfv_multiply_plain(c._h, a[i * words:].data_ptr(), b[i * N:].data_ptr(), p[i * words:].data_ptr(),
                                                   w1.data_ptr(), w1.numel() * 8, stream(torch)) == 0
    for gate in GATES:
        unary = gate == "NOT"
        so = words + 32
        out = torch.full((batch * so,), SENTINEL, dtype=torch.int64, device="cuda")
        c.bfv_logic_gate(gate_id(hg, gate), a, words, None if unary else b, NONE if unary else kind,
                         0 if unary else b.numel() // batch, None if unary else key, out, so, batch, None if unary else ws)
        want = chain_tail(c, hg, torch, True, gate, a, None if unary else b, NONE if unary else kind, p, Q, batch, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(out.view(batch, so)[:, :words].contiguous().view(-1), want), (gate, name, kind)
        assert bool((out.view(batch, so)[:, words:] == SENTINEL).all()), "written past the result"


# ---------------------------------------------------------------------------------------------- truth tables through encryption
def bit_patterns():
    """two items of N / 2 slots each; slots and items together cover the four input pairs"""
    k = np.arange(N // 2)
    x = [(k >> 1) & 1, 1 - ((k >> 1) & 1)]
    y = [k & 1, (k >> 2) & 1]
    return x, y


_ckks = {}


def ckks_setup(hg, torch, name):
    if name not in _ckks:
        c, primes = context(hg, hg.CKKS, *SETS[name])
        rng = hg.Rng(77)
        sk = c.generate_secret_key(rng)
        pk = c.generate_public_key(rng, sk)
        rk = c.generate_relin_key(rng, sk)
        scale = float(2 ** (primes[1].bit_length()))
        torch.cuda.synchronize()
        _ckks[name] = dict(c=c, primes=primes, rng=rng, sk=sk, pk=pk, rk=rk, scale=scale)
    return _ckks[name]


def ckks_bits(s, torch, bits):
    c = s["c"]
    plain = [c.ckks_encode(torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda(), s["scale"]) for v in bits]
    ct = [c.ckks_encrypt(s["rng"], s["pk"], p) for p in plain]
    return torch.cat(ct), torch.cat(plain)


def ckks_values(s, torch, ct, limbs, scale, batch):
    c = s["c"]
    depth = c.Q_size - limbs
    out = []
    for i in range(batch):
        item = ct[i * 2 * limbs * N:(i + 1) * 2 * limbs * N].contiguous()
        out.append(c.ckks_decode(c.ckks_decrypt(item, s["sk"], depth), scale, depth).cpu().numpy())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(SETS))
def test_ckks_truth_tables(hg, torch, name):
    """Every gate, ciphertext and plaintext second operand: decrypt, decode, round to the nearest integer.  No tolerance is
    tuned: a bit is right exactly when the error of its slot is below 0.5.  Largest error observed on an MI355X (the
    printed line): 9.900e-05 for method_I at scale 2^30, 2.271e-06 for method_II at scale 2^36."""
    s = ckks_setup(hg, torch, name)
    c, primes, scale = s["c"], s["primes"], s["scale"]
    Q, batch = c.Q_size, 2
    x, y = bit_patterns()
    assert {(int(p), int(q)) for i in range(2) for p, q in zip(x[i], y[i])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ca, _ = ckks_bits(s, torch, x)
    cb, pb = ckks_bits(s, torch, y)
    ws = c.workspace(hg.OP_CKKS_LOGIC_GATE, 0, batch)
    worst = 0.0
    for gate in GATES:
        for kind in ([NONE] if gate == "NOT" else [CIPHER, PLAIN]):
            unary = gate == "NOT"
            limbs = Q if unary else Q - 1
            out = torch.empty(batch * 2 * limbs * N, dtype=torch.int64, device="cuda")
            b, bs = {NONE: (None, 0), CIPHER: (cb, 2 * Q * N), PLAIN: (pb, Q * N)}[kind]
            c.ckks_logic_gate(gate_id(hg, gate), ca, 2 * Q * N, b, kind, bs, s["rk"] if kind == CIPHER else None, scale, out,
                              2 * limbs * N, 0, batch, None if unary else ws)
            # the metadata rule of the class layer: the product's scale for AND / NAND, the first operand's otherwise
            out_scale = scale * scale / primes[Q - 1] if gate in ("AND", "NAND") else scale
            got = ckks_values(s, torch, out, limbs, out_scale, batch)
            for i in range(batch):
                want = 1 - x[i] if unary else TABLE[gate](x[i], y[i])
                err = float(np.max(np.abs(got[i] - want)))
                worst = max(worst, err)
                assert np.array_equal(np.rint(got[i]).astype(np.int64), want), (gate, kind, i, err)
    print(f"CKKS truth tables {name}: largest error {worst:.3e} (scale 2^{int(np.log2(scale))})")
    assert worst < 0.5


def test_ckks_full_adder(hg, torch):
    """sum = a ^ b ^ cin, carry = (a & b) | (cin & (a ^ b)) at scale 2^30 on the six-prime method I chain; an operand above
    the level a gate needs is mod_dropped (a host-side copy of its first limbs).  All eight input rows, one per slot.
    Largest error observed on an MI355X: 1.448e-04 on the sum, 7.520e-05 on the carry."""
    s = ckks_setup(hg, torch, "method_I")
    c, scale = s["c"], s["scale"]
    assert scale == 2.0 ** 30
    Q = c.Q_size
    k = np.arange(N // 2)
    a, b, cin = (k >> 2) & 1, (k >> 1) & 1, k & 1
    (ca, _), (cb, _), (cc, _) = (ckks_bits(s, torch, [v]) for v in (a, b, cin))

    def gate(name, u, v, limbs):
        depth = Q - limbs
        out = torch.empty(2 * (limbs - 1) * N, dtype=torch.int64, device="cuda")
        c.ckks_logic_gate(gate_id(hg, name), u, 0, v, CIPHER, 0, s["rk"], scale, out, 0, depth, 1,
                          c.workspace(hg.OP_CKKS_LOGIC_GATE, depth, 1))
        return out

    x = gate("XOR", ca, cb, Q)                                     # depth 1
    total = gate("XOR", x, drop(cc, 1, Q, Q - 1), Q - 1)           # depth 2
    ab = gate("AND", ca, cb, Q)                                    # depth 1
    cx = gate("AND", drop(cc, 1, Q, Q - 1), x, Q - 1)              # depth 2
    carry = gate("OR", drop(ab, 1, Q - 1, Q - 2), cx, Q - 2)       # depth 3
    got_sum = ckks_values(s, torch, total, Q - 2, scale, 1)[0]
    got_carry = ckks_values(s, torch, carry, Q - 3, scale, 1)[0]
    want_sum, want_carry = a ^ b ^ cin, (a & b) | (cin & (a ^ b))
    print(f"CKKS full adder: largest error sum {np.max(np.abs(got_sum - want_sum)):.3e}, "
          f"carry {np.max(np.abs(got_carry - want_carry)):.3e}")
    assert np.array_equal(np.rint(got_sum).astype(np.int64), want_sum)
    assert np.array_equal(np.rint(got_carry).astype(np.int64), want_carry)
    assert len({(int(p), int(q), int(r)) for p, q, r in zip(a[:8], b[:8], cin[:8])}) == 8


_bfv = {}


def bfv_setup(hg, torch, log_q, log_p):
    key = (tuple(log_q), tuple(log_p))
    if key not in _bfv:
        c, primes = context(hg, hg.BFV, log_q, log_p)
        rng = hg.Rng(78)
        sk = c.generate_secret_key(rng)
        pk = c.generate_public_key(rng, sk)
        rk = c.generate_relin_key(rng, sk)
        torch.cuda.synchronize()
        _bfv[key] = dict(c=c, rng=rng, sk=sk, pk=pk, rk=rk)
    return _bfv[key]


def bfv_bits(s, torch, bits):
    c = s["c"]
    plain = [c.bfv_encode(torch.from_numpy(np.asarray(v, dtype=np.int64)).cuda()) for v in bits]
    return torch.cat([c.bfv_encrypt(s["rng"], s["pk"], p) for p in plain]), torch.cat(plain)


def bfv_values(s, torch, ct, batch):
    c = s["c"]
    words = 2 * c.Q_size * N
    out = [c.bfv_decode(c.bfv_decrypt(ct[i * words:(i + 1) * words].contiguous(), s["sk"])).cpu().numpy() for i in range(batch)]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(BFV_SETS))
def test_bfv_truth_tables(hg, torch, name):
    s = bfv_setup(hg, torch, *BFV_SETS[name])
    c, batch = s["c"], 2
    words = 2 * c.Q_size * N
    k = np.arange(N)
    x, y = [(k >> 1) & 1, 1 - ((k >> 1) & 1)], [k & 1, (k >> 2) & 1]
    ca, _ = bfv_bits(s, torch, x)
    cb, pb = bfv_bits(s, torch, y)
    ws = c.workspace(hg.OP_BFV_LOGIC_GATE, 0, batch)
    for gate in GATES:
        for kind in ([NONE] if gate == "NOT" else [CIPHER, PLAIN]):
            unary = gate == "NOT"
            out = torch.empty(batch * words, dtype=torch.int64, device="cuda")
            b, bs = {NONE: (None, 0), CIPHER: (cb, words), PLAIN: (pb, N)}[kind]
            c.bfv_logic_gate(gate_id(hg, gate), ca, words, b, kind, bs, s["rk"] if kind == CIPHER else None, out, words, batch,
                             None if unary else ws)
            got = bfv_values(s, torch, out, batch)
            for i in range(batch):
                want = 1 - x[i] if unary else TABLE[gate](x[i], y[i])
                assert np.array_equal(got[i], want), (gate, kind, i)


def test_bfv_full_adder(hg, torch):
    s = bfv_setup(hg, torch, *BFV_DEEP)
    c = s["c"]
    words = 2 * c.Q_size * N
    k = np.arange(N)
    a, b, cin = (k >> 2) & 1, (k >> 1) & 1, k & 1
    (ca, _), (cb, _), (cc, _) = (bfv_bits(s, torch, [v]) for v in (a, b, cin))
    ws = c.workspace(hg.OP_BFV_LOGIC_GATE, 0, 1)

    def gate(name, u, v):
        out = torch.empty(words, dtype=torch.int64, device="cuda")
        c.bfv_logic_gate(gate_id(hg, name), u, 0, v, CIPHER, 0, s["rk"], out, 0, 1, ws)
        return out

    x = gate("XOR", ca, cb)
    total = gate("XOR", x, cc)
    carry = gate("OR", gate("AND", ca, cb), gate("AND", cc, x))
    assert np.array_equal(bfv_values(s, torch, total, 1)[0], a ^ b ^ cin)
    assert np.array_equal(bfv_values(s, torch, carry, 1)[0], (a & b) | (cin & (a ^ b)))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_queue_nothing(hg, torch):
    c, primes = context(hg, hg.CKKS, *SETS["method_I"])
    bfv, _ = context(hg, hg.BFV, *BFV_SETS["method_I"])
    Q = c.Q_size
    l = Q
    a = hg.to_device(synth_ct(primes, range(l), 2, N, 1))
    b = hg.to_device(synth_ct(primes, range(l), 2, N, 2))
    p = hg.to_device(synth_ct(primes, range(l - 1), 2, N, 3))
    key = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 3))
    ws = c.workspace(hg.OP_CKKS_LOGIC_GATE, 0, 1)
    out = torch.full((2 * l * N,), SENTINEL, dtype=torch.int64, device="cuda")
    s = 2.0 ** 30
    w, wl = 2 * l * N, 2 * (l - 1) * N

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), "a refusal wrote to out"

    X = hg.LOGIC_XOR
    refused(lambda: c.ckks_gate_combine(7, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, out, wl, l - 1))             # bad gate
    refused(lambda: c.ckks_gate_combine(X, a, w, l - 2, b, CIPHER, w, l, p, wl, l - 1, s, out, wl, l - 1))         # a below limbs
    refused(lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l - 2, p, wl, l - 1, s, out, wl, l - 1))         # b below limbs
    refused(lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 2, s, out, wl, l - 1))             # p below limbs
    refused(lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, out, 0, l - 1, batch=32768))  # oversized batch
    refused(lambda: bfv.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, out, wl, l - 1))           # wrong scheme
    refused(lambda: c.bfv_gate_combine(X, a, w, b, CIPHER, w, p, w, out, w))                                       # wrong scheme
    refused(lambda: c.ckks_logic_gate(9, a, w, b, CIPHER, w, key, s, out, wl, 0, 1, ws))                           # bad gate
    refused(lambda: c.ckks_logic_gate(X, a, w, b, CIPHER, w, key, s, out, wl, 0, 1, ws[:ws.numel() - 1]))          # short workspace
    refused(lambda: c.ckks_logic_gate(X, a, w, b, CIPHER, w, key, s, out, wl, Q - 1, 1, ws))                       # last level
    refused(lambda: c.ckks_logic_gate(X, a, w, b, CIPHER, w, None, s, out, wl, 0, 1, ws))                          # no key
    refused(lambda: bfv.ckks_logic_gate(X, a, w, b, CIPHER, w, key, s, out, wl, 0, 1, ws))                         # wrong scheme
    refused(lambda: c.bfv_logic_gate(X, a, w, b, CIPHER, w, key, out, w, 1, ws))                                   # wrong scheme
    # forbidden aliasing: the operands are the watched buffers here
    before_a, before_b = a.clone(), b.clone()
    for fn in (lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, a, w, l - 1),             # a has more limbs
               lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, b[N:], w, l - 1),         # shifted into b
               lambda: c.ckks_gate_combine(X, a, w, l, b, CIPHER, w, l, p, wl, l - 1, s, p, wl, l - 1),            # the product
               lambda: c.ckks_logic_gate(X, a, w, b, CIPHER, w, key, s, a, wl, 0, 1, ws)):
        refused(fn)
        assert torch.equal(a, before_a) and torch.equal(b, before_b)
