"""Polynomial evaluation on CKKS ciphertexts: hegpu_ckks_weighted_sum, hegpu_ckks_double_sub and hegpu_ckks_poly_eval
(DESIGN.md 4.5c).  Every comparison is exact: against Python integers, against the chain of single entries the new kernels
replace, and against the same plan executed step by step with entries that exist without them (multiply, relinearize,
rescale, gaussian_integer_op, constant_op, addition).

The key-switch sets are those of test_gpu_mpc.py (method I: one special prime, method II: two) with their chains
lengthened to six primes: a polynomial of degree 7 at depth 1 needs five levels, the sets there have four and three.
"""
import numpy as np
import pytest

from heongpu_amd import api
from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
SETS = {"method_I": ([50, 30, 30, 30, 30, 30], [50]), "method_II": ([36, 36, 36, 36, 36, 36], [37, 37])}
LONG = ([60, 40, 40, 40, 40, 40, 40, 40], [60])
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_contexts = {}


def context(hg, log_q, log_p):
    key = (tuple(log_q), tuple(log_p))
    if key not in _contexts:
        c = hg.Context.from_bit_sizes(hg.CKKS, N, list(log_q), list(log_p), sec=hg.SEC_NONE)
        c.upload()
        _contexts[key] = (c, [int(x) for x in c.table("modulus")])
    return _contexts[key]


def slot_constants(w, q, psi):
    """the residues of round(re) +- round(im) psi^(N/2) on the two halves of the NTT positions"""
    re, im = int(round(complex(w).real)), int(round(complex(w).imag))
    return (re + im * psi) % q, (re - im * psi) % q


def weighted_sum_model(terms, term_limbs, weights, w0, limbs, primes, psi_half):
    """terms: host arrays [2][L_k][N]; -> [2][limbs][N] with Python integers"""
    out = np.zeros((2, limbs, N), dtype=np.uint64)
    for j in range(limbs):
        q, psi = primes[j], int(psi_half[j])
        for p in range(2):
            acc = np.zeros(N, dtype=object)
            for t, L, w in zip(terms, term_limbs, weights):
                first, second = slot_constants(w, q, psi)
                k = np.array([first] * (N // 2) + [second] * (N // 2), dtype=object)
                acc = acc + t.reshape(2, L, N)[p, j].astype(object) * k
            if p == 0:
                first, second = slot_constants(w0, q, psi)
                acc = acc + np.array([first] * (N // 2) + [second] * (N // 2), dtype=object)
            out[p, j] = np.array(acc % q, dtype=np.uint64)
    return out


def padded(torch, hg, items, pad):
    """items: host arrays of equal length -> (device tensor with sentinel padding, stride, offset of item 0)"""
    words = len(items[0])
    stride = words + pad
    buf = np.full(pad + stride * len(items), SENTINEL, dtype=np.uint64)
    for b, it in enumerate(items):
        buf[pad + b * stride: pad + b * stride + words] = it
    return hg.to_device(buf), stride, pad


def make_terms(primes, k, limbs, seed, maximal=False):
    term_limbs = [limbs + (2 if i % 2 else 0) for i in range(k)]
    terms = []
    for i, L in enumerate(term_limbs):
        per_item = []
        for b in range(2):
            if maximal:
                per_item.append(np.concatenate([np.full(N, primes[j] - 1, dtype=np.uint64) for _ in range(2) for j in range(L)]))
            else:
                per_item.append(synth_ct(primes, range(L), 2, N, seed + 10 * i + b))
        terms.append(per_item)
    return terms, term_limbs


@pytest.mark.parametrize("kind", ["real", "complex", "maximal"])
@pytest.mark.parametrize("limbs", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 15])
def test_weighted_sum_against_python_integers(hg, torch, k, limbs, kind):
    """batch 2, padded strides, sentinels around out; 'maximal': every residue q - 1 and every weight = -1 = q - 1 (mod q),
    the largest sum the 128-bit bound allows, on a chain whose first prime has 60 bits"""
    c, primes = context(hg, [60, 40, 40, 40, 40], [60])
    assert primes[0].bit_length() >= 60
    psi_half = c.table("psi_half")
    rng = np.random.default_rng(k * 10 + limbs)
    terms, term_limbs = make_terms(primes, k, limbs, 77, maximal=kind == "maximal")
    if kind == "maximal":
        weights, w0 = [-1.0] * k, -1.0
    elif kind == "real":
        weights, w0 = [float(v) for v in rng.integers(-2 ** 40, 2 ** 40, k)], float(rng.integers(-2 ** 50, 2 ** 50))
    else:
        weights = [complex(a, b) for a, b in zip(rng.integers(-2 ** 40, 2 ** 40, k), rng.integers(-2 ** 40, 2 ** 40, k))]
        w0 = complex(float(2 ** 80 + 12345 * 2 ** 30), -float(2 ** 41 + 1))
    dev = [padded(torch, hg, t, 64 + 2 * i) for i, t in enumerate(terms)]
    out_words = 2 * limbs * N
    out, so, off = padded(torch, hg, [np.full(out_words, SENTINEL, dtype=np.uint64)] * 2, 128)
    c.ckks_weighted_sum([d[0][d[2]:] for d in dev], [d[1] for d in dev], term_limbs, weights, w0, out[off:], so, limbs, batch=2)
    torch.cuda.synchronize()
    got = hg.to_host(out)
    for b in range(2):
        want = weighted_sum_model([t[b] for t in terms], term_limbs, weights, w0, limbs, primes, psi_half)
        assert np.array_equal(got[off + b * so: off + b * so + out_words], want.reshape(-1)), (k, limbs, kind, b)
    mask = np.ones(len(got), dtype=bool)
    for b in range(2):
        mask[off + b * so: off + b * so + out_words] = False
    assert np.all(got[mask] == SENTINEL), "a word outside out was written"


def drop(t, batch, limbs_in, limbs):
    """the first `limbs` limbs of both parts of a contiguous batch [batch][2][limbs_in][N]: always a copy (mod_drop), so
    that the in-place entries of a chain never write into a register that is read again"""
    return t.view(batch, 2, limbs_in, N)[:, :, :limbs].clone().reshape(-1)


def chain_weighted_sum(c, torch, terms, term_limbs, weights, w0, limbs, batch):
    """gaussian_integer_op (multiply) per term on its first `limbs` limbs, hegpu_addition, gaussian_integer_op (add)"""
    words = 2 * limbs * N
    acc = torch.zeros(batch * words, dtype=torch.int64, device="cuda")
    for t, L, w in zip(terms, term_limbs, weights):
        d = drop(t, batch, L, limbs)
        for b in range(batch):
            c.ckks_gaussian_integer_op(1, d[b * words:], complex(w).real, complex(w).imag, limbs, 2, out=d[b * words:])
        c.addition(acc, d, acc, limbs, 2, batch)
    for b in range(batch):
        c.ckks_gaussian_integer_op(0, acc[b * words:], complex(w0).real, complex(w0).imag, limbs, 2, out=acc[b * words:])
    return acc


@pytest.mark.parametrize("k,limbs", [(1, 1), (3, 3), (15, 3), (0, 2)])
def test_weighted_sum_equals_its_chain(hg, torch, k, limbs):
    c, primes = context(hg, [60, 40, 40, 40, 40], [60])
    rng = np.random.default_rng(5 + k)
    terms, term_limbs = make_terms(primes, k, limbs, 300)
    dev = [hg.to_device(np.concatenate(t)) for t in terms]
    weights = [complex(float(a), float(b)) for a, b in zip(rng.integers(-2 ** 45, 2 ** 45, k), rng.integers(-2 ** 45, 2 ** 45, k))]
    w0 = complex(-float(2 ** 79), 3.0)
    out = torch.empty(2 * 2 * limbs * N, dtype=torch.int64, device="cuda")
    c.ckks_weighted_sum(dev, [2 * L * N for L in term_limbs], term_limbs, weights, w0, out, 2 * limbs * N, limbs, batch=2)
    want = chain_weighted_sum(c, torch, dev, term_limbs, weights, w0, limbs, 2)
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("form", ["ciphertext", "ciphertext_higher", "constant", "constant_negative", "in_place",
                                  "in_place_constant"])
def test_double_sub_equals_its_chain(hg, torch, form):
    """addition(a, a) then a subtraction, or constant_op(HEGPU_CONST_SUB)"""
    c, primes = context(hg, [60, 40, 40, 40, 40], [60])
    limbs, batch = 3, 2
    words = 2 * limbs * N
    a_limbs = limbs if form.startswith("in_place") else limbs + 1
    b_limbs = limbs + 2 if form == "ciphertext_higher" else limbs
    a = hg.to_device(np.concatenate([synth_ct(primes, range(a_limbs), 2, N, 40 + b) for b in range(batch)]))
    with_b = form in ("ciphertext", "ciphertext_higher", "in_place")
    b_ct = hg.to_device(np.concatenate([synth_ct(primes, range(b_limbs), 2, N, 50 + b) for b in range(batch)])) if with_b else None
    value = {"constant": 2.0 ** 40 + 0.5, "constant_negative": -(2.0 ** 70), "in_place_constant": 1099511627777.0}.get(form, 0.0)
    # the chain
    a2 = drop(a, batch, a_limbs, limbs)
    c.addition(a2, a2, a2, limbs, 2, batch)
    if with_b:
        c.addition(a2, drop(b_ct, batch, b_limbs, limbs), a2, limbs, 2, batch, op=1)
    else:
        for b in range(batch):
            c.ckks_constant_op(1, a2[b * words:], value, limbs, 2, out=a2[b * words:])
    out = a if form.startswith("in_place") else torch.empty(batch * words, dtype=torch.int64, device="cuda")
    c.ckks_double_sub(a, 2 * a_limbs * N, a_limbs, b_ct, 2 * b_limbs * N if with_b else 0, b_limbs if with_b else 0, value,
                      out, words, limbs, batch=batch)
    torch.cuda.synchronize()
    assert torch.equal(out, a2)


def compose(c, hg, torch, plan, ct, key, depth, batch):
    """the plan with entries that exist without the evaluator; registers are contiguous batches [batch][2][limbs][N]"""
    Q = c.Q_size
    regs = [(ct, Q - depth)]

    def product(x, y, ml):
        l = ml + 1
        xa, ya = drop(x[0], batch, x[1], l), drop(y[0], batch, y[1], l)
        prod = torch.empty(batch * 3 * l * N, dtype=torch.int64, device="cuda")
        c.ckks_multiply(xa, 2 * l * N, ya, 2 * l * N, prod, 3 * l * N, Q - l, batch)
        c.ckks_relinearize_inplace(prod, 3 * l * N, key, Q - l, batch, c.workspace(hg.OP_CKKS_RELIN, Q - l, batch))
        return prod

    def rescaled(t, stride, l):
        c.ckks_rescale_inplace(t, stride, Q - l, batch, c.workspace(hg.OP_CKKS_RESCALE, Q - l, batch))
        return t.view(batch, stride)[:, :2 * (l - 1) * N].contiguous().view(-1), l - 1

    for s in plan.steps:
        limbs = s.level + 1
        words = 2 * limbs * N
        if s.kind == api.POLY_POWER:
            l = s.mul_level + 1
            r, rl = rescaled(product(regs[s.a], regs[s.b], s.mul_level), 3 * l * N, l)
            if s.c != api.POLY_TAIL_NONE:
                r = drop(r, batch, rl, limbs)
                c.addition(r, r, r, limbs, 2, batch)
                if s.c == api.POLY_TAIL_ONE:
                    for b in range(batch):
                        c.ckks_constant_op(1, r[b * words:], s.tail_const, limbs, 2, out=r[b * words:])
                else:
                    c.addition(r, drop(regs[s.c][0], batch, regs[s.c][1], limbs), r, limbs, 2, batch, op=1)
            regs.append((r, limbs))
        elif s.kind == api.POLY_LEAF:
            terms = [regs[s.term_reg[i]] for i in range(s.n_terms)]
            r = chain_weighted_sum(c, torch, [t[0] for t in terms], [t[1] for t in terms],
                                   [complex(s.w[i][0], s.w[i][1]) for i in range(s.n_terms)], complex(s.w0[0], s.w0[1]),
                                   limbs, batch)
            regs.append((r, limbs))
        else:
            q = regs[s.a]
            if s.rescale_first:
                q = rescaled(q[0].clone(), 2 * q[1] * N, q[1])
            l = s.mul_level + 1
            prod = product(q, regs[s.b], s.mul_level).view(batch, 3 * l * N)[:, :2 * l * N].contiguous().view(-1)
            sum_limbs = limbs + s.rescale_after
            r = drop(prod, batch, l, sum_limbs)
            c.addition(r, drop(regs[s.c][0], batch, regs[s.c][1], sum_limbs), r, sum_limbs, 2, batch)
            if s.rescale_after:
                r, _ = rescaled(r, 2 * sum_limbs * N, sum_limbs)
            regs.append((r, limbs))
    return regs[-1][0]


def run_poly_eval(hg, torch, log_q, log_p, basis, degree, depth, batch, seed):
    c, primes = context(hg, log_q, log_p)
    Q, Qp = c.Q_size, c.Q_prime_size
    rng = np.random.default_rng(seed)
    coeffs = rng.uniform(-1, 1, degree + 1) + (1j * rng.uniform(-1, 1, degree + 1) if seed % 2 else 0)
    scale = float(primes[1])
    plan = hg.poly_eval_plan(basis, coeffs, Q - 1 - depth, scale, scale, primes[:Q])
    l = Q - depth
    ct = hg.to_device(np.concatenate([synth_ct(primes, range(l), 2, N, seed + b) for b in range(batch)]))
    key = hg.to_device(synth_key(primes, c.switch_key_digits(), Qp, N, 3))
    so = 2 * plan.out_limbs * N + 32
    out = torch.full((batch * so,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.poly_eval_workspace_bytes(plan, depth, batch) // 8, dtype=torch.int64, device="cuda")
    assert ws.numel() > 0
    c.ckks_poly_eval(ct, 2 * l * N, out, so, plan, key, depth, batch, ws)
    want = compose(c, hg, torch, plan, ct, key, depth, batch)
    torch.cuda.synchronize()
    words = 2 * (plan.level + 1) * N
    assert torch.equal(out.view(batch, so)[:, :words].contiguous().view(-1), want), (basis, degree, depth, batch)
    assert bool((out.view(batch, so)[:, 2 * plan.out_limbs * N:] == 0x5A5A5A5A5A5A5A5A).all()), "written past the result"
    return c, plan, ct, key, out, so, ws


@pytest.mark.parametrize("depth,batch", [(0, 1), (1, 2)])
@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("basis", [api.MONOMIAL, api.CHEBYSHEV])
@pytest.mark.parametrize("name", list(SETS))
def test_poly_eval_equals_the_step_by_step_composition(hg, torch, name, basis, degree, depth, batch):
    run_poly_eval(hg, torch, *SETS[name], basis, degree, depth, batch, 11 + degree + batch)


@pytest.mark.parametrize("degree", [12, 31])
@pytest.mark.parametrize("basis", [api.MONOMIAL, api.CHEBYSHEV])
def test_poly_eval_longer_chain(hg, torch, basis, degree):
    """eight moduli: the lead_ branches and powers at differing levels"""
    run_poly_eval(hg, torch, *LONG, basis, degree, 0, 1, 100 + degree)


def test_refusals_queue_nothing(hg, torch):
    c, plan, ct, key, out, so, ws = run_poly_eval(hg, torch, *SETS["method_I"], api.CHEBYSHEV, 3, 0, 1, 21)
    l = c.Q_size
    out.fill_(0x5A5A5A5A5A5A5A5A)

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A5A5A5A5A5A5A).all()), "a refusal wrote to out"

    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, out, so, plan, key, 0, 1, ws[:ws.numel() - 1]))      # workspace
    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, out, so, plan, key, 1, 1, ws))                       # levels above the input's
    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, out, so, plan, None, 0, 1, ws))                      # null key
    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, None, so, plan, key, 0, 1, ws))                      # null out
    bad = type(plan.steps).from_buffer_copy(plan.steps)
    bad[0].a = 7
    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, out, so, plan._replace(steps=bad), key, 0, 1, ws))   # register out of range
    bad = type(plan.steps).from_buffer_copy(plan.steps)
    bad[len(bad) - 1].level = l
    refused(lambda: c.ckks_poly_eval(ct, 2 * l * N, out, so, plan._replace(steps=bad), key, 0, 1, ws))   # level out of range
    # out overlapping ct
    with pytest.raises(hg.HEError) as e:
        c.ckks_poly_eval(ct, 2 * l * N, ct[N:], so, plan, key, 0, 1, ws)
    assert e.value.code == hg.E_INVALID
    # the kernels' own refusals
    t = ct
    refused(lambda: c.ckks_weighted_sum([t] * 16, [0] * 16, [l] * 16, [1.0] * 16, 0.0, out, so, 2))
    refused(lambda: c.ckks_weighted_sum([t], [0], [1], [1.0], 0.0, out, so, 2))                          # term below the sum
    refused(lambda: c.ckks_weighted_sum([t], [0], [l], [float("nan")], 0.0, out, so, 2))
    refused(lambda: c.ckks_double_sub(t, 0, 1, None, 0, 0, 1.0, out, so, 2))                             # a below the sum
    refused(lambda: c.ckks_double_sub(t, 0, l, None, 0, 0, float("inf"), out, so, 2))
    with pytest.raises(hg.HEError):
        c.ckks_weighted_sum([t], [0], [l], [1.0], 0.0, t[N:], so, 2)                                     # out overlaps a term
    with pytest.raises(hg.HEError):
        c.ckks_double_sub(t, 0, l, None, 0, 0, 1.0, t[N:], so, 2)                                        # overlap, not in place


SEMANTIC = ([60, 40, 40, 40, 40, 40, 40, 40], [60])  # [60, 40 x 7 | 60]
_semantic = {}


def semantic_setup(hg, torch):
    """keys, 2048 values of [-1, 1] encrypted at scale 2^40: made once, shared, left unchanged"""
    if not _semantic:
        c, primes = context(hg, *SEMANTIC)
        rng = hg.Rng(2024)
        sk = c.generate_secret_key(rng)
        pk = c.generate_public_key(rng, sk)
        rk = c.generate_relin_key(rng, sk)
        x = np.random.default_rng(3).uniform(-1, 1, N // 2)
        ct = c.ckks_encrypt(rng, pk, c.ckks_encode(torch.from_numpy(x).cuda(), 2.0 ** 40))
        torch.cuda.synchronize()
        _semantic.update(c=c, primes=primes, sk=sk, rk=rk, x=x, ct=ct)
    return _semantic


SEMANTIC_CASES = {
    "chebyshev_31_sigmoid": (api.CHEBYSHEV, lambda: np.polynomial.chebyshev.Chebyshev.interpolate(
        lambda t: 1.0 / (1.0 + np.exp(-4.0 * t)), 31).coef),
    "monomial_7": (api.MONOMIAL, lambda: np.array([0.5, -0.25, 0.125, 0.75, -0.5, 0.3, -0.2, 0.1])),
}


@pytest.mark.parametrize("case", sorted(SEMANTIC_CASES))
def test_poly_eval_semantics(hg, torch, case):
    """Encrypt, evaluate, decrypt, decode at the plan's final scale, compare with numpy.  The bound is not a constant:
    the step-by-step composition (entries that exist without the evaluator) is measured on the same ciphertext and the
    fused entry must stay within 8 x its error -- the factor covers the spread of encryption noise across seeds; the
    residues of the two are equal anyway (asserted too).  Measured on an MI355X: chebyshev_31_sigmoid composition 1.771e-08,
    fused 1.771e-08, asserted bound 1.417e-07; monomial_7 composition 2.116e-08, fused 2.116e-08, asserted bound 1.693e-07.
    (The composition's own error is also held below 1e-2: values are of size 1, so that only says it computes the polynomial.)"""
    s = semantic_setup(hg, torch)
    c, primes, x = s["c"], s["primes"], s["x"]
    basis, make = SEMANTIC_CASES[case]
    coeffs = make()
    Q = c.Q_size
    plan = hg.poly_eval_plan(basis, coeffs, Q - 1, 2.0 ** 40, 2.0 ** 40, primes[:Q])
    want = (np.polynomial.chebyshev.chebval(x, coeffs) if basis == api.CHEBYSHEV else np.polynomial.polynomial.polyval(x, coeffs))
    depth = Q - 1 - plan.level

    def error(ct):
        got = c.ckks_decode(c.ckks_decrypt(ct, s["sk"], depth), plan.scale, depth)
        torch.cuda.synchronize()
        return float(np.max(np.abs(got.cpu().numpy() - want)))

    composed = compose(c, hg, torch, plan, s["ct"], s["rk"], 0, 1)
    out = torch.empty(2 * plan.out_limbs * N, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.poly_eval_workspace_bytes(plan, 0, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_poly_eval(s["ct"], 2 * Q * N, out, 0, plan, s["rk"], 0, 1, ws)
    fused = out[:2 * (plan.level + 1) * N].contiguous()
    e_comp, e_fused = error(composed), error(fused)
    print(f"{case}: composition {e_comp:.3e}, fused {e_fused:.3e}, bound {8 * e_comp:.3e}, depth {depth}, "
          f"log2 scale {np.log2(plan.scale):.6f}")
    assert torch.equal(fused, composed)
    assert e_comp < 1e-2, "the composition itself does not compute the polynomial"
    assert e_fused <= 8 * e_comp
