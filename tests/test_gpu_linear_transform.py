"""Plaintext matrix x encrypted vector by diagonals (hegpu_ckks_diag_mac, hegpu_ckks_linear_transform).

  1. the one-pass kernel against Python integers, on 60-bit moduli so that the 128-bit sum of 16 products is
     actually approached (every input q - 1 at n1 = 16 is the largest sum it must hold): exact;
  2. the fused entry against the composition of the existing entries (rotate_hoisted, cipherplain_multiplication +
     addition per diagonal, apply_galois per giant step, addition) on the same keys and inputs, methods I and II,
     depth 0 and 1, batch 1 and 2: exact -- both sides are canonical residues of the same integers;
  3. semantics: encrypt v, transform, rescale, decrypt, decode against numpy's M v under the reference tests' own
     criterion |a - b| < 1e-4 (test/test_ckks_relinearization.cpp:9-34).  The margin is derived: with ten diagonals
     the encoding and key-switch error at scale 2^40 is of order N 2^-40 = 2^-28 per term, several orders below
     1e-4 = 2^-13.3; a wrong diagonal or shift convention gives an error of order 1;
  4. refusals: HEGPU_E_INVALID and an untouched result buffer.
"""
import ctypes

import numpy as np
import pytest

from helpers import synth_ct, synth_key
from oracle import binding as ob
from test_gpu_mpc import CKKS_SETS

pytestmark = pytest.mark.gpu

N = 4096
SLOTS = N // 2
DIAGS = [0, 1, 2, 3, 5, 8, 13, 21, 100, 2047]
SENT = 0x5555555555555555


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- 1. kernel against Python integers
@pytest.fixture(scope="module")
def wide(hg, torch):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [60, 60, 60], [60], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    assert all(p.bit_length() == 60 for p in primes)
    c.upload()
    return c, primes


def _want_diag_mac(rot, diags, index, primes, l):
    """rot [n1][2][l][N], diags [n_diag][l][N] -> [n2][2][l][N], Python integers"""
    out = np.zeros((len(index), 2, l, N), dtype=np.uint64)
    for j, row in enumerate(index):
        for p in range(2):
            for y in range(l):
                acc = np.zeros(N, dtype=object)
                for i, at in enumerate(row):
                    if at >= 0:
                        acc = acc + diags[at, y].astype(object) * rot[i, p, y].astype(object)
                out[j, p, y] = np.array(acc % primes[y], dtype=np.uint64)
    return out


def _run_diag_mac(hg, torch, c, primes, l, index, n_diag, fill, batch=2, pad=3 * N):
    n1, n2, depth = len(index[0]), len(index), 3 - l
    words = 2 * l * N
    rs, os_ = n1 * words + pad, n2 * words + pad // 3
    if fill == "max":
        limb = np.stack([np.full(N, primes[y] - 1, dtype=np.uint64) for y in range(l)])
        rot = np.broadcast_to(limb, (batch, n1, 2, l, N)).copy()
        diags = np.broadcast_to(limb, (n_diag, l, N)).copy()
    else:
        rot = np.stack([np.stack([synth_ct(primes, range(l), 2, N, 40 + 100 * b + i).reshape(2, l, N) for i in range(n1)])
                        for b in range(batch)])
        diags = np.stack([synth_ct(primes, range(l), 1, N, 900 + d).reshape(l, N) for d in range(n_diag)])
    rbuf = np.full(batch * rs, SENT, dtype=np.uint64)
    for b in range(batch):
        rbuf[b * rs:b * rs + n1 * words] = rot[b].reshape(-1)
    out = torch.full((batch * os_,), SENT, dtype=torch.int64, device="cuda")
    c.ckks_diag_mac(hg.to_device(rbuf), rs, n1, hg.to_device(diags.reshape(-1)), n_diag, index, n2, out, os_, depth, batch)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, os_)
    for b in range(batch):
        want = _want_diag_mac(rot[b], diags, index, primes, l)
        assert np.array_equal(got[b, :n2 * words], want.reshape(-1)), (l, n1, n2, b)
        assert np.all(got[b, n2 * words:] == SENT), "the padding between the items is untouched"


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("n1,n2", [(1, 1), (3, 2), (16, 2)])
def test_diag_mac_against_python_integers(hg, torch, wide, l, n1, n2):
    c, primes = wide
    rng = np.random.default_rng(n1 * 100 + n2 * 10 + l)
    n_diag = n1 * n2
    perm = rng.permutation(n_diag)
    index = [[int(perm[j * n1 + i]) for i in range(n1)] for j in range(n2)]
    if n1 > 1:  # a few holes in the last row, the first stays full
        for i in rng.choice(n1, size=n1 // 3, replace=False):
            index[-1][i] = -1
    _run_diag_mac(hg, torch, c, primes, l, index, n_diag, "random")


@pytest.mark.parametrize("l", [1, 3])
def test_diag_mac_absent_row_and_single_entry(hg, torch, wide, l):
    c, primes = wide
    index = [[0, 1, 2], [-1, -1, -1], [-1, 3, -1]]  # full, entirely absent (zeros), one entry
    _run_diag_mac(hg, torch, c, primes, l, index, 4, "random")


def test_diag_mac_largest_sum(hg, torch, wide):
    """every input q - 1 at n1 = 16: sixteen products of (q - 1)^2, the largest value the accumulator must hold"""
    c, primes = wide
    index = [list(range(16)), list(range(15, -1, -1))]
    _run_diag_mac(hg, torch, c, primes, 3, index, 16, "max")


# ---------------------------------------------------------------- 2. fused entry against the composition
_SETS = {}


def _set(hg, name):
    if name not in _SETS:
        log_q, log_p = CKKS_SETS[name]
        c = hg.Context.from_bit_sizes(hg.CKKS, N, log_q, log_p, sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        c.upload()
        _SETS[name] = (c, primes, {})
    return _SETS[name]


def _key(hg, entry, shift):
    c, primes, keys = entry
    if shift not in keys:
        keys[shift] = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 7 + shift))
    return keys[shift]


def _composition(hg, torch, c, ct, cs, diags, plan, bkeys, belts, gkeys, gelts, depth, batch):
    """the same transform from the existing C-ABI entries; returns [batch][2 l N]"""
    l = c.Q_size - depth
    words = 2 * l * N
    st = torch.cuda.current_stream().cuda_stream
    lib = c._lib
    rot = torch.empty(batch * plan.n1 * words, dtype=torch.int64, device="cuda")
    c.ckks_rotate_hoisted(ct, cs, rot, plan.n1 * words, bkeys, belts, depth, batch, c.workspace(hg.OP_CKKS_GALOIS, depth, batch))
    rot = rot.reshape(batch, plan.n1, words)
    ws = c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
    total = None
    for j, row in enumerate(plan.index):
        inner = None
        for i, at in enumerate(row):
            if at < 0:
                continue
            prod = torch.empty(batch * words, dtype=torch.int64, device="cuda")
            for b in range(batch):
                rc = lib.hegpu_cipherplain_multiplication(c._h, rot[b, i].data_ptr(), diags[at].data_ptr(),
                                                          prod.data_ptr() + b * words * 8, l, st)
                assert rc == 0
            if inner is None:
                inner = prod
            else:
                c.addition(inner, prod, inner, l, 2, batch)
        assert inner is not None
        if gelts[j]:
            turned = torch.empty_like(inner)
            c.ckks_apply_galois(inner, words, turned, words, gkeys[j], gelts[j], depth, batch, ws)
            inner = turned
        if total is None:
            total = inner
        else:
            c.addition(total, inner, total, l, 2, batch)
    torch.cuda.synchronize()
    return hg.to_host(total).reshape(batch, words)


PLANS = {"ten_diagonals_n1_4": (DIAGS, 4), "giant_steps_only": ([0, 1, 5, 2047], 1), "baby_steps_only": ([0, 1, 3], 4)}


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_fused_entry_equals_the_composition(hg, torch, name, depth, batch):
    entry = _set(hg, name)
    c, primes, _ = entry
    l = c.Q_size - depth
    words = 2 * l * N
    cs = words + N  # items further apart than their payload
    cts = [synth_ct(primes, range(l), 2, N, 300 + b) for b in range(batch)]
    cbuf = np.full(batch * cs, SENT, dtype=np.uint64)
    for b in range(batch):
        cbuf[b * cs:b * cs + words] = cts[b]
    ct = hg.to_device(cbuf)
    for plan_name, (ks, period) in PLANS.items():
        plan = hg.linear_transform_plan(ks, SLOTS, period)
        if plan_name == "giant_steps_only":
            assert plan.n1 == 1 and plan.baby_shifts == [0]
        if plan_name == "baby_steps_only":
            assert plan.n2 == 1 and plan.giant_shifts == [0]
        n_diag = len(ks)
        diags = hg.to_device(np.concatenate([synth_ct(primes, range(l), 1, N, 600 + d) for d in range(n_diag)])).reshape(n_diag, l * N)
        belts = [hg.steps_to_galois_elt(s, N, 5) if s else 0 for s in plan.baby_shifts]
        gelts = [hg.steps_to_galois_elt(s, N, 5) if s else 0 for s in plan.giant_shifts]
        bkeys = [_key(hg, entry, s) if s else None for s in plan.baby_shifts]
        gkeys = [_key(hg, entry, s) if s else None for s in plan.giant_shifts]
        so = words + 2 * N
        out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
        nbytes = c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, batch)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
        c.ckks_linear_transform(ct, cs, out, so, diags, n_diag, plan.index, bkeys, belts, gkeys, gelts, depth, batch, ws)
        torch.cuda.synchronize()
        got = hg.to_host(out).reshape(batch, so)
        want = _composition(hg, torch, c, ct, cs, diags, plan, bkeys, belts, gkeys, gelts, depth, batch)
        for b in range(batch):
            assert np.array_equal(got[b, :words], want[b]), (name, plan_name, depth, batch, b)
            assert np.all(got[b, words:] == SENT), "the padding between the items is untouched"
        assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"


# ---------------------------------------------------------------- 3. semantics
def test_transform_of_an_encrypted_vector_is_the_matrix_product(hg, torch):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [60, 40, 40], [60], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    Q = c.Q_size
    words = 2 * Q * N
    scale = 2.0 ** 40
    rnd = np.random.default_rng(11)
    v = rnd.uniform(-1, 1, SLOTS)
    diag = {k: rnd.uniform(-1, 1, SLOTS) for k in DIAGS}
    plan = hg.linear_transform_plan(DIAGS, SLOTS)
    rng = hg.Rng(2024)
    sk = c.generate_secret_key(rng)
    pk = c.generate_public_key(rng, sk)
    shifts = sorted({s for s in plan.baby_shifts + plan.giant_shifts if s})
    keys = {s: c.generate_galois_key(rng, sk, hg.steps_to_galois_elt(s, N, 5)) for s in shifts}
    ct = c.ckks_encrypt(rng, pk, c.ckks_encode(torch.from_numpy(v).cuda(), scale))
    # diagonal k = j n1 + i is rotated by pre_rotation = -j n1 before encoding; rot(x, s) = numpy.roll(x, -s)
    packed = torch.cat([c.ckks_encode(torch.from_numpy(np.roll(diag[k], -plan.pre_rotation[p])).cuda(), scale)
                        for p, k in enumerate(sorted(DIAGS))])
    belts = [hg.steps_to_galois_elt(s, N, 5) if s else 0 for s in plan.baby_shifts]
    gelts = [hg.steps_to_galois_elt(s, N, 5) if s else 0 for s in plan.giant_shifts]
    out = torch.empty(words, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(plan.n1, plan.n2, 0, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_linear_transform(ct, words, out, words, packed, len(DIAGS), plan.index, [keys.get(s) for s in plan.baby_shifts],
                            belts, [keys.get(s) for s in plan.giant_shifts], gelts, 0, 1, ws)
    c.ckks_rescale_inplace(out, words, 0, 1, c.workspace(hg.OP_CKKS_RESCALE, 0, 1))
    plain = c.ckks_decrypt(out, sk, depth=1)
    got = c.ckks_decode(plain, scale * scale / primes[Q - 1], depth=1).cpu().numpy()
    m = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for k in DIAGS:
        m[s, (s + k) % SLOTS] += diag[k]
    err = np.abs(got - m @ v).max()
    print(f"max |decode - M v| = {err:.3e} (criterion 1e-4)")
    assert err < 1e-4


# ---------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(hg, torch):
    entry = _set(hg, "method_I")
    c, primes, _ = entry
    l = c.Q_size
    words = 2 * l * N
    g = hg.steps_to_galois_elt(1, N, 5)
    key = _key(hg, entry, 1)
    ct = hg.to_device(synth_ct(primes, range(l), 2, N, 1))
    diags = hg.to_device(synth_ct(primes, range(l), 1, N, 2))
    buf = torch.full((words,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(16, 2, 0, 1) // 8, dtype=torch.int64, device="cuda")

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote its result buffer"

    # n1 = 17
    refused(lambda: c.ckks_linear_transform(ct, words, buf, words, diags, 1, [[0] + [-1] * 16], [None] + [key] * 16,
                                            [0] + [g] * 16, [None], [0], 0, 1, ws))
    refused(lambda: c.ckks_diag_mac(ct, words, 17, diags, 1, [[0] + [-1] * 16], 1, buf, words, 0, 1))
    # an index >= n_diag, one below -1
    refused(lambda: c.ckks_linear_transform(ct, words, buf, words, diags, 1, [[1]], [None], [0], [None], [0], 0, 1, ws))
    refused(lambda: c.ckks_diag_mac(ct, words, 1, diags, 1, [[-2]], 1, buf, words, 0, 1))
    # a short workspace
    short = ws[:c.linear_transform_workspace_bytes(1, 2, 0, 1) // 8 - 1]
    refused(lambda: c.ckks_linear_transform(ct, words, buf, words, diags, 1, [[0], [0]], [None], [0], [None, key], [0, g],
                                            0, 1, short))
    # out overlapping ct (the last word of the input is the first of the result); rot overlapping out
    both = torch.full((2 * words,), SENT, dtype=torch.int64, device="cuda")
    for view in (both[words - 1:2 * words - 1], both[:words]):
        with pytest.raises(hg.HEError) as e:
            c.ckks_linear_transform(both[:words], words, view, words, diags, 1, [[0]], [None], [0], [None], [0], 0, 1, ws)
        assert e.value.code == hg.E_INVALID
        with pytest.raises(hg.HEError) as e:
            c.ckks_diag_mac(both[:words], words, 1, diags, 1, [[0]], 1, view, words, 0, 1)
        assert e.value.code == hg.E_INVALID
    torch.cuda.synchronize()
    assert bool((both == SENT).all())
    # the same calls with valid arguments go through
    c.ckks_linear_transform(ct, words, buf, words, diags, 1, [[0], [0]], [None], [0], [None, key], [0, g], 0, 1, ws)
    torch.cuda.synchronize()
    assert not bool((buf == SENT).all())
