"""The modulus raise of CKKS bootstrapping on the device (csrc/rns.hip k_mod_raise, csrc/ops.cpp op_ckks_mod_raise).

hegpu_mod_raise is compared word for word with `lift` below, the reference's mod_raise_kernel (src/lib/kernel/
bootstrapping.cu:339-376) restated on integers: a coefficient v of the q_0 limb stands for c = v - q_0 when v >= q_0 >> 1,
else for v; limb 0 is v, limb j is |c| mod q_j for c >= 0 and q_j - (|c| mod q_j) for c < 0 -- the WORD q_j when q_j
divides |c|.  hegpu_ckks_mod_raise (NTT domain in and out, the lift as the load transform of the forward pass) is compared
bit for bit with the chain hegpu_ntt (inverse) -> hegpu_mod_raise -> hegpu_ntt (forward), whose transform canonicalises
that word to 0.  Every launch form of the decomposing transform is reached through the context options that force it, so
the shapes stay small."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4096
CHAINS = {
    "wide_source": ([60, 40, 30, 50, 60], [60]),   # 60-bit q_0 into 30 bits: outside the Barrett domain
    "fp64_source": ([40, 60, 50, 36], [60]),       # targets larger than the source
    "two_limbs": ([50, 40], [50]),
}
SENTINEL = 0x5A5A5A5A5A5A5A5A
_contexts = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def context(hg, name, n=N):
    key = (name, n)
    if key not in _contexts:
        log_q, log_p = CHAINS[name] if name in CHAINS else ([60, 50, 50, 60], [60])
        c = hg.Context.from_bit_sizes(hg.CKKS, n, log_q, log_p, sec=hg.SEC_NONE)
        c.upload()
        _contexts[key] = (c, [int(v) for v in c.table("modulus")][:len(log_q)])
    return _contexts[key]


def lift(v, q0, qj):
    """limb j > 0 of the reference's kernel for the uint64 array v of residues modulo q0"""
    neg = v >= np.uint64(q0 >> 1)
    mag = np.where(neg, np.uint64(q0) - v, v)
    r = mag % np.uint64(qj)
    return np.where(neg, np.uint64(qj) - r, r)


def planted(primes, parts, batch, n, seed):
    """[batch][parts][n] residues modulo q_0: the edge values first, one polynomial of q_0 - 1, the rest random"""
    q0 = primes[0]
    h = (q0 - 1) // 2
    rng = np.random.default_rng(seed)
    v = rng.integers(0, q0, size=(batch, parts, n), dtype=np.uint64)
    edge = [0, 1, h - 1, h, h + 1, q0 - 1]
    for qj in primes[1:]:
        for k in (1, 2, 3, q0 // qj):
            if 0 < k * qj < q0:
                edge += [q0 - k * qj, k * qj]  # c = -k q_j (the word q_j) and c = +k q_j (0), when they fall on those sides
    e = np.array(edge, dtype=np.uint64)
    for b in range(batch):
        for p in range(parts):
            v[b, p, (b + p):(b + p) + len(e)] = e
            v[b, p, n - len(e):] = e
    v[batch - 1, parts - 1, :] = q0 - 1
    return v


def want_raise(v, primes, limbs):
    out = np.empty(v.shape[:2] + (limbs, v.shape[2]), dtype=np.uint64)
    out[:, :, 0, :] = v
    for j in range(1, limbs):
        out[:, :, j, :] = lift(v, primes[0], primes[j])
    return out


def test_lift_writes_the_word_q_j(hg):
    """the model itself: a negative multiple of q_j gives q_j, a positive one 0"""
    _, primes = context(hg, "wide_source")
    q0, q1 = primes[0], primes[1]
    v = np.array([q0 - q1, q1, q0 - 1, (q0 - 1) // 2, (q0 - 1) // 2 - 1], dtype=np.uint64)
    assert [int(x) for x in lift(v, q0, q1)] == [q1, 0, q1 - 1, q1 - ((q0 + 1) // 2) % q1, ((q0 - 1) // 2 - 1) % q1]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_mod_raise_words(hg, torch, chain, parts, batch):
    c, primes = context(hg, chain)
    Q = len(primes)
    v = planted(primes, parts, batch, N, 7 * parts + batch)
    for limbs in sorted({Q, 1, 2}):
        in_stride, out_stride, pad = parts * N + 512, parts * limbs * N + 1024, 512
        src = torch.full((batch * in_stride,), -1, dtype=torch.int64, device="cuda")
        src.view(batch, in_stride)[:, :parts * N] = hg.to_device(v.reshape(batch, parts * N))
        out = torch.full((pad + batch * out_stride,), SENTINEL, dtype=torch.int64, device="cuda")
        c.mod_raise(src, in_stride, out[pad:], out_stride, limbs, parts, batch)
        torch.cuda.synchronize()
        got = hg.to_host(out)
        assert np.all(got[:pad] == SENTINEL)
        body = got[pad:].reshape(batch, out_stride)
        assert np.all(body[:, parts * limbs * N:] == SENTINEL)  # the padding between items and behind the last
        want = want_raise(v, primes, limbs).reshape(batch, parts * limbs * N)
        assert np.array_equal(body[:, :parts * limbs * N], want), (chain, parts, batch, limbs)


def ckks_case(hg, torch, c, primes, n, out_depth, batch, seed):
    Q = len(primes)
    L = Q - out_depth
    v = planted(primes, 2, batch, n, seed)
    coef = hg.to_device(v.reshape(-1))
    ct = torch.empty_like(coef)
    c.ntt(coef, ct, False, 2 * batch, 1)                      # the planted values carried to the NTT domain
    # the chain of three entries
    back = torch.empty_like(ct)
    c.ntt(ct, back, True, 2 * batch, 1)
    raised = torch.empty(batch * 2 * L * n, dtype=torch.int64, device="cuda")
    c.mod_raise(back, 2 * n, raised, 2 * L * n, L, 2, batch)
    want = torch.empty_like(raised)
    c.ntt(raised, want, False, 2 * L * batch, L)
    # the operator, padded strides, exactly workspace_bytes bytes with a guard word behind
    cs, so, pad = 2 * n + 256, 2 * L * n + 768, 256
    src = torch.full((batch * cs,), -1, dtype=torch.int64, device="cuda")
    src.view(batch, cs)[:, :2 * n] = ct.view(batch, 2 * n)
    out = torch.full((pad + batch * so,), SENTINEL, dtype=torch.int64, device="cuda")
    nbytes = c.workspace_bytes(hg.OP_CKKS_MOD_RAISE, out_depth, batch)
    assert nbytes == 2 * n * 8 * batch
    wsbuf = torch.full((nbytes // 8 + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    c.ckks_mod_raise(src, cs, out[pad:], so, out_depth, batch, wsbuf, ws_bytes=nbytes)
    torch.cuda.synchronize()
    assert int(wsbuf[-1].item()) == SENTINEL
    assert torch.equal(src.view(batch, cs)[:, :2 * n], ct.view(batch, 2 * n))  # the input is read only
    got = out[pad:].view(batch, so)
    assert bool(torch.all(out[:pad] == SENTINEL)) and bool(torch.all(got[:, 2 * L * n:] == SENTINEL))
    assert torch.equal(got[:, :2 * L * n], want.view(batch, 2 * L * n))
    w = hg.to_host(want).reshape(batch, 2, L, n)
    assert all(int(w[:, :, j].max()) < primes[j] for j in range(L))  # canonical: the word q_j became 0
    assert np.array_equal(w[:, :, 0].reshape(-1), hg.to_host(ct))    # limb 0 is the input limb


# the launch forms of the decomposing forward transform: by launch size, the two passes, the multi-modulus column pass
# (with the inverse column stages of an FP64 source inside it), and that pass without the fused inverse
FORMS = {"auto": {}, "two_pass": {"single_pass": 0}, "single_pass": {"single_pass": 1}, "col_multi": {"col_multi": 1},
         "col_multi_own_inverse": {"col_multi": 1, "fuse_inverse": 0}}


def with_options(c, options, fn):
    before = {k: c.get_option(k) for k in options}
    try:
        for k, val in options.items():
            c.set_option(k, val)
        fn()
    finally:
        for k, val in before.items():
            c.set_option(k, val)


@pytest.mark.parametrize("form", ["auto", "two_pass", "col_multi", "col_multi_own_inverse"])
@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("out_depth", [0, 1])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_ckks_mod_raise_is_the_chain(hg, torch, chain, out_depth, batch, form):
    c, primes = context(hg, chain)
    with_options(c, FORMS[form], lambda: ckks_case(hg, torch, c, primes, N, out_depth, batch, 11 * batch + out_depth))


@pytest.mark.parametrize("n,batch,form", [
    (1 << 13, 2, "auto"), (1 << 13, 2, "single_pass"), (1 << 13, 1, "col_multi"),
    (1 << 14, 1, "auto"), (1 << 14, 2, "single_pass"), (1 << 14, 2, "col_multi"),
    (1 << 15, 2, "auto"), (1 << 15, 1, "col_multi"),
    (1 << 16, 1, "auto"), (1 << 16, 2, "col_multi"), (1 << 16, 1, "col_multi_own_inverse")])
def test_ckks_mod_raise_every_degree(hg, torch, n, batch, form):
    """each degree takes other kernels: one LDS-resident pass up to 2^14 (by launch size; forced here), two passes above,
    and at 2^16 the multi-modulus column pass that takes the integer targets along"""
    c, primes = context(hg, "degrees", n)
    with_options(c, FORMS[form], lambda: ckks_case(hg, torch, c, primes, n, 0, batch, n % 1000 + batch))


def test_last_depth_is_a_copy(hg, torch):
    c, primes = context(hg, "wide_source")
    ckks_case(hg, torch, c, primes, N, len(primes) - 1, 2, 5)


def test_refusals_leave_the_output_untouched(hg, torch):
    c, primes = context(hg, "wide_source")
    Q = len(primes)
    src = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
    out = torch.full((2 * Q * N,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = c.workspace(hg.OP_CKKS_MOD_RAISE, 0, 1)
    calls = [
        lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q + 1, 2, 1),
        lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, 0, 2, 1),
        lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 4, 1),
        lambda: c.mod_raise(src, 2 * N, out, 2 * Q * N, Q, 2, 0),
        lambda: c.mod_raise(None, 2 * N, out, 2 * Q * N, Q, 2, 1),
        lambda: c.mod_raise(out[N:], 2 * N, out, 2 * Q * N, Q, 2, 1),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, Q, 1, ws),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, -1, 1, ws),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 0, ws),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, ws, ws_bytes=2 * N * 8 - 8),
        lambda: c.ckks_mod_raise(out[N:], 2 * N, out, 2 * Q * N, 0, 1, ws),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, out[4 * N:], ws_bytes=2 * N * 8),
        lambda: c.ckks_mod_raise(src, 2 * N, out, 2 * Q * N, 0, 1, src, ws_bytes=2 * N * 8),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(hg.HEError) as e:
            call()
        assert e.value.code == hg.E_INVALID, i
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL)) and bool(torch.all(src == 0))
