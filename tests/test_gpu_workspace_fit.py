"""Every operator sequence stays inside the workspace its size query reports.

Each case allocates 2 x need bytes in ONE buffer: the first half is the workspace, handed to the entry with ws_bytes = need
exactly, the second half is filled with a sentinel.  Asserted: (a) the guard half is unchanged, and (b) the output is
bit-identical to the same call with a separate workspace of 2 x need bytes.  The guard lies inside the same allocation, so
a sequence that carves its workspace differently from what the size query reports fails an assertion instead of faulting.

N = 4096, batch 2, item strides larger than the items.  The parameter sets are those of tests/test_workspace_sizes.py."""
import ctypes

import numpy as np
import pytest

from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
BATCH = 2
PAD = N  # words between the items of a batch
SENTINEL = 0x5A5A5A5A5A5A5A5A
CKKS_SETS = {"I": ([40, 30, 30], [40]), "II_p2": ([40, 35, 35, 35, 35], [40, 40]), "II_p3": ([40, 35, 35, 35, 35], [40, 41, 40])}
BFV_SETS = {"I": ([36, 36, 36], [37]), "II": ([36, 36, 36], [37, 37])}
T = 65537


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def contexts(hg):
    """(scheme, name) -> (context, primes, relinearisation / Galois key), made once per parameter set, left unchanged and
    released with the module"""
    made = {}

    def get(scheme, name):
        if (scheme, name) not in made:
            bfv = scheme == "bfv"
            log_q, log_p = (BFV_SETS if bfv else CKKS_SETS)[name]
            c = hg.Context.from_bit_sizes(hg.BFV if bfv else hg.CKKS, N, log_q, log_p, plain_modulus=T if bfv else 0,
                                          sec=hg.SEC_NONE)
            primes = [int(x) for x in c.table("modulus")]
            c.upload()
            key = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 3))
            made[(scheme, name)] = (c, primes, key)
        return made[(scheme, name)]

    yield get
    made.clear()


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def batch_of(hg, primes, limbs, parts, seed):
    """BATCH synthetic items [parts][limbs][N], PAD words apart -> (device tensor, stride)"""
    words = parts * limbs * N
    buf = np.full(BATCH * (words + PAD), SENTINEL, dtype=np.uint64)
    for b in range(BATCH):
        buf[b * (words + PAD): b * (words + PAD) + words] = synth_ct(primes, range(limbs), parts, N, seed + b)
    return hg.to_device(buf), words + PAD


def fits(torch, need, run):
    """run(ws) -> the entry's output, a new tensor on every call.  Returns the output of the tight call."""
    assert need > 0 and need % 8 == 0
    words = need // 8
    buf = torch.empty(2 * words, dtype=torch.int64, device="cuda")
    buf[words:] = SENTINEL
    got = run(buf[:words])
    torch.cuda.synchronize()
    assert bool((buf[words:] == SENTINEL).all()), "written past the reported workspace size"
    want = run(torch.empty(2 * words, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got, want), "the result depends on the room behind the workspace"
    return got


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_ckks_relinearize(hg, torch, contexts, name, depth):
    c, primes, key = contexts("ckks", name)
    l = c.Q_size - depth
    prod, stride = batch_of(hg, primes, l, 3, 10)

    def run(ws):
        ct = prod.clone()
        c.ckks_relinearize_inplace(ct, stride, key, depth, BATCH, ws)
        return ct

    fits(torch, c.workspace_bytes(hg.OP_CKKS_RELIN, depth, BATCH), run)


@pytest.mark.parametrize("depth", [0, 1])
def test_ckks_rescale(hg, torch, contexts, depth):
    c, primes, _ = contexts("ckks", "I")
    src, stride = batch_of(hg, primes, c.Q_size - depth, 2, 20)

    def run(ws):
        ct = src.clone()
        c.ckks_rescale_inplace(ct, stride, depth, BATCH, ws)
        return ct

    fits(torch, c.workspace_bytes(hg.OP_CKKS_RESCALE, depth, BATCH), run)


def galois(c, torch, hg, src, stride, key, elt, depth, ws):
    out = torch.full_like(src, SENTINEL)
    c.ckks_apply_galois(src, stride, out, stride, key, elt, depth, BATCH, ws)
    return out


@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_ckks_apply_galois(hg, torch, contexts, name, depth):
    c, primes, key = contexts("ckks", name)
    src, stride = batch_of(hg, primes, c.Q_size - depth, 2, 30)
    fits(torch, c.workspace_bytes(hg.OP_CKKS_GALOIS, depth, BATCH), lambda ws: galois(c, torch, hg, src, stride, key, 5, depth, ws))


@pytest.mark.parametrize("op", ["OP_CKKS_GALOIS", "OP_CKKS_ROTATE_HOISTED"], ids=["one_accumulator", "four_accumulators"])
@pytest.mark.parametrize("name", ["I", "II_p2"])
def test_ckks_rotate_hoisted(hg, torch, contexts, name, op):
    c, primes, key = contexts("ckks", name)
    depth, elts = 0, [5, 0, 25]
    l = c.Q_size - depth
    words = 2 * l * N
    src, stride = batch_of(hg, primes, l, 2, 40)
    so = len(elts) * words + PAD

    def run(ws):
        out = torch.full((BATCH * so,), SENTINEL, dtype=torch.int64, device="cuda")
        c.ckks_rotate_hoisted(src, stride, out, so, [key if e else None for e in elts], elts, depth, BATCH, ws)
        return out

    # The guarded run has exactly the named row.  The comparison run's 2 x need bytes hold four accumulators in both
    # cases, so for one_accumulator the two runs take different paths: their outputs must be bit-identical all the same.
    got = fits(torch, c.workspace_bytes(getattr(hg, op), depth, BATCH), run).view(BATCH, so)
    assert bool((got[:, len(elts) * words:] == SENTINEL).all())
    ws = c.workspace(hg.OP_CKKS_GALOIS, depth, BATCH)
    for i, e in enumerate(elts):
        want = galois(c, torch, hg, src, stride, key, e, depth, ws) if e else src
        torch.cuda.synchronize()
        assert torch.equal(got[:, i * words:(i + 1) * words], want.view(BATCH, stride)[:, :words]), (name, op, e)


@pytest.mark.parametrize("name", list(BFV_SETS))
def test_bfv_multiply_relinearize_galois(hg, torch, contexts, name):
    c, primes, key = contexts("bfv", name)
    Q = c.Q_size
    a, stride = batch_of(hg, primes, Q, 2, 50)
    b, _ = batch_of(hg, primes, Q, 2, 60)
    ps = 3 * Q * N + PAD

    def multiply(ws):
        out = torch.full((BATCH * ps,), SENTINEL, dtype=torch.int64, device="cuda")
        c.bfv_multiply(a, stride, b, stride, out, ps, BATCH, ws)
        return out

    prod = fits(torch, c.workspace_bytes(hg.OP_BFV_MULTIPLY, 0, BATCH), multiply)

    def relinearize(ws):
        ct = prod.clone()
        c.bfv_relinearize_inplace(ct, ps, key, BATCH, ws)
        return ct

    fits(torch, c.workspace_bytes(hg.OP_BFV_RELIN, 0, BATCH), relinearize)

    def rotate(ws):
        out = torch.full_like(a, SENTINEL)
        c.bfv_apply_galois(a, stride, out, stride, key, 5, BATCH, ws)
        return out

    fits(torch, c.workspace_bytes(hg.OP_BFV_GALOIS, 0, BATCH), rotate)


@pytest.mark.parametrize("name", ["I", "II_p2"])
def test_ckks_linear_transform(hg, torch, contexts, name):
    """n1 = n2 = 2: one baby rotation, one giant rotation, every region of the composite workspace in use"""
    c, primes, key = contexts("ckks", name)
    depth = 0
    l = c.Q_size - depth
    src, stride = batch_of(hg, primes, l, 2, 70)
    diags = hg.to_device(np.concatenate([synth_ct(primes, range(l), 1, N, 600 + d) for d in range(4)]))
    belts, gelts = [0, hg.steps_to_galois_elt(1, N, 5)], [0, hg.steps_to_galois_elt(2, N, 5)]

    def run(ws):
        out = torch.full_like(src, SENTINEL)
        c.ckks_linear_transform(src, stride, out, stride, diags, 4, [[0, 1], [2, 3]], [None, key], belts, [None, key], gelts,
                                depth, BATCH, ws)
        return out

    fits(torch, c.linear_transform_workspace_bytes(2, 2, depth, BATCH), run)


def test_ckks_poly_eval(hg, torch, contexts):
    """the degree-7 monomial plan of tests/test_workspace_sizes.py on the five-prime chain"""
    from test_workspace_sizes import poly_plans
    c, primes, key = contexts("ckks", "II_p2")
    plan = poly_plans(hg, c)["monomial7"]
    src, stride = batch_of(hg, primes, c.Q_size, 2, 80)
    so = 2 * plan.out_limbs * N + PAD

    def run(ws):
        out = torch.full((BATCH * so,), SENTINEL, dtype=torch.int64, device="cuda")
        c.ckks_poly_eval(src, stride, out, so, plan, key, 0, BATCH, ws)
        return out

    fits(torch, c.poly_eval_workspace_bytes(plan, 0, BATCH), run)


def test_ckks_logic_gate(hg, torch, contexts):
    c, primes, key = contexts("ckks", "I")
    l = c.Q_size
    a, stride = batch_of(hg, primes, l, 2, 90)
    b, _ = batch_of(hg, primes, l, 2, 100)
    so = 2 * (l - 1) * N + PAD

    def run(ws):
        out = torch.full((BATCH * so,), SENTINEL, dtype=torch.int64, device="cuda")
        c.ckks_logic_gate(hg.LOGIC_AND, a, stride, b, hg.GATE_B_CIPHER, stride, key, float(primes[1]), out, so, 0, BATCH, ws)
        return out

    fits(torch, c.workspace_bytes(hg.OP_CKKS_LOGIC_GATE, 0, BATCH), run)


def test_bfv_logic_gate(hg, torch, contexts):
    c, primes, key = contexts("bfv", "I")
    a, stride = batch_of(hg, primes, c.Q_size, 2, 110)
    b, _ = batch_of(hg, primes, c.Q_size, 2, 120)

    def run(ws):
        out = torch.full_like(a, SENTINEL)
        c.bfv_logic_gate(hg.LOGIC_AND, a, stride, b, hg.GATE_B_CIPHER, stride, key, out, stride, BATCH, ws)
        return out

    fits(torch, c.workspace_bytes(hg.OP_BFV_LOGIC_GATE, 0, BATCH), run)


@pytest.mark.parametrize("name", ["I", "II_p2"])
def test_ckks_encrypt_and_switch_key(hg, torch, contexts, name):
    """one item each; the generator is seeded anew for every call, so the DRBG makes both calls draw the same"""
    c, primes, _ = contexts("ckks", name)
    Q, Qp = c.Q_size, c.Q_prime_size
    rng = hg.Rng(7)
    sk = c.generate_secret_key(rng)
    pk = c.generate_public_key(rng, sk)
    plain = hg.to_device(synth_ct(primes, range(Q), 1, N, 130))
    torch.cuda.synchronize()

    def encrypt(ws):
        ct = torch.full((2 * Q * N,), SENTINEL, dtype=torch.int64, device="cuda")
        r = hg.Rng(11)
        rc = c._lib.hegpu_ckks_encrypt(c._h, r._h, pk.data_ptr(), plain.data_ptr(), ct.data_ptr(), ws.data_ptr(),
                                       ws.numel() * 8, stream(torch))
        assert rc == 0, c._lib.hegpu_last_error()
        return ct

    fits(torch, c.workspace_bytes(hg.OP_CKKS_ENCRYPT, 0, 1), encrypt)

    def relin_key(ws):
        rk = torch.full((c.switch_key_digits() * 2 * Qp * N,), SENTINEL, dtype=torch.int64, device="cuda")
        r = hg.Rng(12)
        rc = c._lib.hegpu_generate_relin_key(c._h, r._h, sk.data_ptr(), rk.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                             stream(torch))
        assert rc == 0, c._lib.hegpu_last_error()
        return rk

    fits(torch, c.workspace_bytes(hg.OP_KEYGEN_SWITCH, 0, 1), relin_key)


def test_ckks_decode(hg, torch, contexts):
    c, primes, _ = contexts("ckks", "I")
    depth = 1
    plain = hg.to_device(synth_ct(primes, range(c.Q_size - depth), 1, N, 140))

    def run(ws):
        out = torch.zeros(N // 2, dtype=torch.float64, device="cuda")
        rc = c._lib.hegpu_ckks_decode(c._h, plain.data_ptr(), depth, 2.0 ** 30, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                      stream(torch))
        assert rc == 0, c._lib.hegpu_last_error()
        return out.view(torch.int64)  # compared by their bits

    fits(torch, c.workspace_bytes(hg.OP_CKKS_DECODE, depth, 1), run)


def test_bfv_refresh_merge_beyond_one_group_of_shares(hg, torch, contexts):
    """17 shares: the first 16 are summed into the head_sum region of the workspace, behind the rounded plaintexts"""
    c, primes, _ = contexts("bfv", "I")
    Q, k = c.Q_size, 17
    words = 2 * Q * N
    ct, stride = batch_of(hg, primes, Q, 2, 150)
    shares = [hg.to_device(np.concatenate([synth_ct(primes, range(Q), 2, N, 200 + 10 * i + b) for b in range(BATCH)]))
              for i in range(k)]
    arr = (ctypes.c_void_p * k)(*[s.data_ptr() for s in shares])

    def run(ws):
        out = torch.full_like(ct, SENTINEL)
        crs = hg.Rng(4242)
        rc = c._lib.hegpu_mpc_bfv_refresh_merge(c._h, crs._h, ct.data_ptr(), stride, arr, k, out.data_ptr(), stride,
                                                BATCH, ws.data_ptr(), ws.numel() * 8, stream(torch))
        assert rc == 0, c._lib.hegpu_last_error()
        return out

    got = fits(torch, c.workspace_bytes(hg.OP_MPC_REFRESH_MERGE, 0, BATCH), run).view(BATCH, stride)
    assert bool((got[:, words:] == SENTINEL).all()), "the padding between the items is untouched"
