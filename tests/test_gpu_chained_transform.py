"""Chained giant steps of the plaintext matrix x encrypted vector product (hegpu_ckks_linear_transform_chained), N = 4096.

  1. the chained entry against the composition of the single entries in forest order (rotate_hoisted,
     cipherplain_multiplication + addition per diagonal, apply_galois per link, addition), residue for residue: both
     sides are canonical residues of the same integers.  Methods I and II, depth 0 and 1, batch 1 and 2, items further
     apart than their payload, sentinel padding, the input unwritten.  Plans: two-sided dense (offsets -7 .. 7, period
     4: the negative side hangs on giant step 0), one-sided with a gap, no giant step 0 (the root is rotated into the
     result), two roots (no zero shift between a positive and a negative side: the rotated roots are summed), and
     sixteen terms in one chain of depth 15 (batch 1, method I);
  2. an all -1 parent table is hegpu_ckks_linear_transform, bit for bit;
  3. semantics: keys for the REDUCED shift list only; encrypt v, chained transform, rescale, decrypt, decode against
     numpy's M v under the criterion of test_gpu_linear_transform.py, 1e-4 = 2^-13.3: at most 16 chained key switches
     add at most 16 terms of order N 2^-40, about 2^-24.  Without the chained entry the direct transform has no key
     for most of its giant steps;
  4. refusals: HEGPU_E_INVALID and an untouched result buffer;
  5. the entry on a side stream and from a captured graph (helpers.side_stream_and_graph_parity).
"""
import numpy as np
import pytest

from helpers import side_stream_and_graph_parity, synth_ct
from test_gpu_linear_transform import DIAGS, N, SENT, SLOTS, _composition, _key, _set
from test_gpu_mpc import CKKS_SETS

pytestmark = pytest.mark.gpu

# name -> (diagonal offsets, period, batches, key-switch sets)
PLANS = {
    "two_sided_dense": (list(range(-7, 8)), 4, (1, 2), tuple(CKKS_SETS)),
    "one_sided_with_a_gap": (DIAGS, 4, (1, 2), tuple(CKKS_SETS)),
    "no_giant_zero": ([5, 6, 9, 40, 41], 4, (1, 2), tuple(CKKS_SETS)),
    "two_roots": ([-10, -6, -5, 5, 6, 9], 4, (2,), tuple(CKKS_SETS)),
    "sixteen_in_one_chain": (list(range(16)), 1, (1,), ("method_I",)),
}
CASES = [(plan, name, batch) for plan, (_, _, batches, names) in PLANS.items() for name in names for batch in batches]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def elt(hg, shift):
    return hg.steps_to_galois_elt(shift, N, 5) if shift else 0


def chained_arguments(hg, entry, ks, period):
    """plan, chain and the key / element lists of the chained entry, on the synthetic keys of test_gpu_linear_transform"""
    plan = hg.linear_transform_plan(ks, SLOTS, period)
    chain = hg.giant_step_chain(plan.giant_shifts, SLOTS)
    belts = [elt(hg, s) for s in plan.baby_shifts]
    lelts = [elt(hg, s) for s in chain.link_shifts]
    bkeys = [_key(hg, entry, s) if s else None for s in plan.baby_shifts]
    lkeys = [_key(hg, entry, s) if s else None for s in chain.link_shifts]
    return plan, chain, bkeys, belts, lkeys, lelts


def forest_composition(hg, torch, c, ct, cs, diags, plan, bkeys, belts, lkeys, lelts, parent, depth, batch):
    """S_j = inner_j + sum of galois(S_k) over the children, the result = sum of galois(S_r) over the roots, from the
    existing C-ABI entries; returns [batch][2 l N]"""
    l = c.Q_size - depth
    words = 2 * l * N
    st = torch.cuda.current_stream().cuda_stream
    lib = c._lib
    ws = c.workspace(hg.OP_CKKS_GALOIS, depth, batch)
    rot = torch.empty(batch * plan.n1 * words, dtype=torch.int64, device="cuda")
    c.ckks_rotate_hoisted(ct, cs, rot, plan.n1 * words, bkeys, belts, depth, batch, ws)
    rot = rot.reshape(batch, plan.n1, words)
    inners = []
    for row in plan.index:
        inner = torch.zeros(batch * words, dtype=torch.int64, device="cuda")
        for i, at in enumerate(row):
            if at < 0:
                continue
            prod = torch.empty(batch * words, dtype=torch.int64, device="cuda")
            for b in range(batch):
                rc = lib.hegpu_cipherplain_multiplication(c._h, rot[b, i].data_ptr(), diags[at].data_ptr(),
                                                          prod.data_ptr() + b * words * 8, l, st)
                assert rc == 0
            c.addition(inner, prod, inner, l, 2, batch)
        inners.append(inner)

    def turned(x, j):
        if not lelts[j]:
            return x
        y = torch.empty_like(x)
        c.ckks_apply_galois(x, words, y, words, lkeys[j], lelts[j], depth, batch, ws)
        return y

    def folded(j):
        total = inners[j]
        for k in range(plan.n2):
            if parent[k] == j:
                c.addition(total, turned(folded(k), k), total, l, 2, batch)
        return total

    out = torch.zeros(batch * words, dtype=torch.int64, device="cuda")
    for r in range(plan.n2):
        if parent[r] == -1:
            c.addition(out, turned(folded(r), r), out, l, 2, batch)
    torch.cuda.synchronize()
    return hg.to_host(out).reshape(batch, words)


def items(primes, l, batch, seed, pad):
    words = 2 * l * N
    cs = words + pad
    buf = np.full(batch * cs, SENT, dtype=np.uint64)
    for b in range(batch):
        buf[b * cs:b * cs + words] = synth_ct(primes, range(l), 2, N, seed + b)
    return buf, cs


def synthetic_diagonals(hg, primes, l, n_diag):
    host = np.concatenate([synth_ct(primes, range(l), 1, N, 600 + d) for d in range(n_diag)])
    return host, hg.to_device(host).reshape(n_diag, l * N)


# ---------------------------------------------------------------- 1. against the composition in forest order
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("plan_name,name,batch", CASES)
def test_chained_entry_equals_the_composition_in_forest_order(hg, torch, plan_name, name, batch, depth):
    entry = _set(hg, name)
    c, primes, _ = entry
    ks = PLANS[plan_name][0]
    plan, chain, bkeys, belts, lkeys, lelts = chained_arguments(hg, entry, ks, PLANS[plan_name][1])
    if plan_name == "two_sided_dense":
        assert plan.giant_shifts == [0, 4, SLOTS - 8, SLOTS - 4] and chain.parent == [-1, 0, 3, 0]
        assert sorted(set(chain.link_shifts)) == [0, 4, SLOTS - 4]
    if plan_name == "one_sided_with_a_gap":
        assert plan.giant_shifts == [0, 4, 8, 12, 20, 100, SLOTS - 4] and chain.parent == [-1, 0, 1, 2, 3, 4, 0]
        assert chain.link_shifts == [0, 4, 4, 4, 8, 80, SLOTS - 4]
    if plan_name == "no_giant_zero":
        assert plan.giant_shifts == [4, 8, 40] and chain.parent == [-1, 0, 1] and chain.link_shifts[0] == 4
    if plan_name == "two_roots":  # no zero shift to join the two sides: both roots are rotated, then summed
        assert plan.giant_shifts == [4, 8, SLOTS - 12, SLOTS - 8] and chain.parent == [-1, 0, 3, -1]
        assert chain.link_shifts == [4, 4, SLOTS - 4, SLOTS - 8]
    if plan_name == "sixteen_in_one_chain":
        assert plan.n2 == 16 and plan.n1 == 1 and chain.parent == [-1] + list(range(15))
    l = c.Q_size - depth
    words = 2 * l * N
    cbuf, cs = items(primes, l, batch, 300, N)  # items further apart than their payload
    ct = hg.to_device(cbuf)
    n_diag = len(ks)
    _, diags = synthetic_diagonals(hg, primes, l, n_diag)
    so = words + 2 * N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, batch) // 8, dtype=torch.int64, device="cuda")
    c.ckks_linear_transform(ct, cs, out, so, diags, n_diag, plan.index, bkeys, belts, lkeys, lelts, depth, batch, ws,
                            giant_parent=chain.parent)
    torch.cuda.synchronize()
    got = hg.to_host(out).reshape(batch, so)
    want = forest_composition(hg, torch, c, ct, cs, diags, plan, bkeys, belts, lkeys, lelts, chain.parent, depth, batch)
    for b in range(batch):
        assert np.array_equal(got[b, :words], want[b]), (plan_name, name, depth, batch, b)
        assert np.all(got[b, words:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"


# ---------------------------------------------------------------- 2. no parent is the direct entry
@pytest.mark.parametrize("name", list(CKKS_SETS))
def test_a_table_of_roots_is_the_direct_entry(hg, torch, name):
    entry = _set(hg, name)
    c, primes, _ = entry
    depth, batch = 0, 2
    l = c.Q_size - depth
    words = 2 * l * N
    plan = hg.linear_transform_plan(DIAGS, SLOTS, 4)
    belts, gelts = [elt(hg, s) for s in plan.baby_shifts], [elt(hg, s) for s in plan.giant_shifts]
    bkeys = [_key(hg, entry, s) if s else None for s in plan.baby_shifts]
    gkeys = [_key(hg, entry, s) if s else None for s in plan.giant_shifts]
    cbuf, cs = items(primes, l, batch, 310, N)
    ct = hg.to_device(cbuf)
    _, diags = synthetic_diagonals(hg, primes, l, len(DIAGS))
    ws = torch.empty(c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, batch) // 8, dtype=torch.int64, device="cuda")
    outs = []
    for parent in (None, [-1] * plan.n2):
        out = torch.full((batch * words,), SENT, dtype=torch.int64, device="cuda")
        c.ckks_linear_transform(ct, cs, out, words, diags, len(DIAGS), plan.index, bkeys, belts, gkeys, gelts, depth, batch,
                                ws, giant_parent=parent)
        torch.cuda.synchronize()
        outs.append(hg.to_host(out))
    assert np.array_equal(outs[0], outs[1])
    want = _composition(hg, torch, c, ct, cs, diags, plan, bkeys, belts, gkeys, gelts, depth, batch)
    assert np.array_equal(outs[1].reshape(batch, words), want)


# ---------------------------------------------------------------- 3. semantics on the reduced key set
def test_chained_transform_with_the_reduced_keys_is_the_matrix_product(hg, torch):
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
    chain = hg.giant_step_chain(plan.giant_shifts, SLOTS)
    direct = sorted({s for s in plan.baby_shifts + plan.giant_shifts if s})
    reduced = sorted({s for s in plan.baby_shifts + chain.link_shifts if s})
    print("shifts with a key: direct", direct, "chained", reduced)
    assert len(reduced) < len(direct)
    rng = hg.Rng(2024)
    sk = c.generate_secret_key(rng)
    pk = c.generate_public_key(rng, sk)
    keys = {s: c.generate_galois_key(rng, sk, elt(hg, s)) for s in reduced}  # nothing else
    assert any(s and s not in keys for s in plan.giant_shifts), "the direct transform lacks a key here"
    ct = c.ckks_encrypt(rng, pk, c.ckks_encode(torch.from_numpy(v).cuda(), scale))
    # the plan's own pre-rotated diagonals, as in the direct mode; rot(x, s) = numpy.roll(x, -s)
    packed = torch.cat([c.ckks_encode(torch.from_numpy(np.roll(diag[k], -plan.pre_rotation[p])).cuda(), scale)
                        for p, k in enumerate(sorted(DIAGS))])
    lkeys, lelts, parent, links = hg.chained_giant_steps(plan.giant_shifts, N, lambda e: keys[{elt(hg, s): s for s in reduced}[e]])
    assert parent == chain.parent and links == chain.link_shifts
    out = torch.empty(words, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(plan.n1, plan.n2, 0, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_linear_transform(ct, words, out, words, packed, len(DIAGS), plan.index, [keys.get(s) for s in plan.baby_shifts],
                            [elt(hg, s) for s in plan.baby_shifts], lkeys, lelts, 0, 1, ws, giant_parent=parent)
    c.ckks_rescale_inplace(out, words, 0, 1, c.workspace(hg.OP_CKKS_RESCALE, 0, 1))
    got = c.ckks_decode(c.ckks_decrypt(out, sk, depth=1), scale * scale / primes[Q - 1], depth=1).cpu().numpy()
    m = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for k in DIAGS:
        m[s, (s + k) % SLOTS] += diag[k]
    err = np.abs(got - m @ v).max()
    print(f"max |decode - M v| = {err:.3e} (criterion 1e-4), {sum(1 for e in lelts if e)} chained key switches")
    assert err < 1e-4


# ---------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(hg, torch):
    entry = _set(hg, "method_I")
    c, primes, _ = entry
    l = c.Q_size
    words = 2 * l * N
    g = elt(hg, 1)
    key = _key(hg, entry, 1)
    ct = hg.to_device(synth_ct(primes, range(l), 2, N, 1))
    diags = hg.to_device(synth_ct(primes, range(l), 1, N, 2))
    buf = torch.full((words,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.linear_transform_workspace_bytes(1, 3, 0, 1) // 8, dtype=torch.int64, device="cuda")
    index = [[0], [0], [0]]

    def call(parent, keys=(None, key, key), elts=(0, g, g), work=ws):
        c.ckks_linear_transform(ct, words, buf, words, diags, 1, index, [None], [0], list(keys), list(elts), 0, 1, work,
                                giant_parent=parent)

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote its result buffer"

    refused(lambda: call([-1, 2, 1]))   # a cycle
    refused(lambda: call([-1, 1, 0]))   # a term that is its own parent
    refused(lambda: call([-1, 0, 3]))   # a parent equal to n2
    refused(lambda: call([-1, 0, -2]))  # a parent below -1
    # a non-zero link without a key (the shared element-list check names it first); a key is not needed for element 0
    refused(lambda: call([-1, 0, 1], keys=(None, key, None)))
    refused(lambda: call([-1, 0, 1], work=ws[:ws.numel() - 1]))  # a workspace one word short
    # the same calls with valid arguments go through
    call([-1, 0, 1])
    torch.cuda.synchronize()
    assert not bool((buf == SENT).all())
    first = buf.clone()
    call([-1, 0, 1], keys=(None, key, None), elts=(0, g, 0))
    torch.cuda.synchronize()
    assert not bool((buf == first).all())


# ---------------------------------------------------------------- 5. side stream and captured graph
def test_chained_entry_on_a_side_stream_and_from_a_graph(hg, torch):
    """two-sided, offsets -5 .. 5 with period 4: the composition in forest order that
    test_chained_entry_equals_the_composition_in_forest_order pins the entry to"""
    B = 2
    entry = _set(hg, "method_I")
    c, primes, _ = entry
    depth = 0
    l = c.Q_size - depth
    words = 2 * l * N
    ks = list(range(-5, 6))
    plan, chain, bkeys, belts, lkeys, lelts = chained_arguments(hg, entry, ks, 4)
    assert any(p != -1 for p in chain.parent)
    n_diag = len(ks)
    host_diags, diags = synthetic_diagonals(hg, primes, l, n_diag)

    def case(seed):
        cts = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        want = forest_composition(hg, torch, c, hg.to_device(np.concatenate(cts)), words, diags, plan, bkeys, belts, lkeys,
                                  lelts, chain.parent, depth, B)
        return {"ct": cts}, {"out": list(want)}

    zeros = [np.zeros(words, dtype=np.uint64) for _ in range(B)]
    nbytes = c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, B)
    operands = {"ct": (zeros, "in"), "diags": ([host_diags], "in"), "out": (zeros, "out"),
                "ws": ([np.zeros(nbytes // 8, dtype=np.uint64)], "ws")}
    call = lambda d, s: c.ckks_linear_transform(d["ct"], s["ct"], d["out"], s["out"], d["diags"], n_diag, plan.index,  # noqa: E731
                                                bkeys, belts, lkeys, lelts, depth, B, d["ws"], giant_parent=chain.parent)
    side_stream_and_graph_parity(torch, operands, call, [case(seed) for seed in (3, 8)])
