"""The slim, bit and gate refreshes (hegpu_ckks_slim_bootstrap over heongpu_amd.api.slim_bootstrap_plan), N = 4096,
three pieces each way, degree 30, r = 3, K = 12.

  1. the entry against the chain of single entries (hegpu_addition for a gate's two inputs, per SlotToCoeff factor
     hegpu_ckks_linear_transform + _rescale_inplace, hegpu_ckks_mod_raise, per CoeffToSlot factor the same pair,
     hegpu_ckks_apply_galois with 2N - 1, hegpu_ckks_conj_real, hegpu_ckks_poly_eval at batch B) on synthetic keys, diagonals
     and inputs: exact.  Chains A, B and A with method II of tests/test_gpu_bootstrap.py, batch 1 and 2, the arithmetic
     plan without ct2 and the AND plan with ct2.  The padding between items and a guard word behind the workspace are
     untouched, the inputs are not written.
  2. encrypted accuracy with real keys and a secret of Hamming weight 32.  First the precondition: every |t| / q_0 of the
     raise, and with it every overflow I, is below K (decrypted on the host from the chain's raised ciphertext).
       slim   chain A, scale 2^40, ratio 256: real slots uniform(-0.5, 0.5) and the eight-value pattern;
              max |decode - f(z)| < 1e-4 over all 2048 slots, f(z) = (rho / 2 pi) sin(2 pi z / rho), rho = 256: the
              criterion of this repository's semantic tests, the one DESIGN.md 4.5f asserts;
       bit    {42, 41 x 17 | 60}, scale 2^41 (q_0 = 2 scale, as the reference's example): bits with a deliberate error e
              uniform in +-0.02 added before encoding; max |decode - b| <= (pi 0.02)^2 / 4 + 1e-4.  The first term is the
              exact bound 1/2 (1 - cos pi e) <= (pi e)^2 / 4: a wrong function or phase fails by about 0.5 while the
              input's own 0.02 passes;
       gates  the first 18 primes of the reference's gate example (q_0 = 3 * 2^40) | one of its special primes, scale
              2^40: all four input pairs spread over the slots, all six gates; every bit is right and the error < 1e-4.
  3. refusals launch nothing.
The measured figures are printed and recorded in DESIGN.md 4.5g."""
import numpy as np
import pytest

from helpers import synth_ct, synth_key
from test_gpu_bootstrap import CHAINS, overflow_of_the_raise

pytestmark = pytest.mark.gpu

N = 4096
SLOTS = N // 2
SENT = 0x5555555555555555
K = 12
GATE_Q = [3298535538689, 1099512938497, 1099515691009, 1099516870657, 1099521458177, 1099522375681, 1099523555329,
          1099525128193, 1099526176769, 1099529060353, 1099535220737, 1099536138241, 1099537580033, 1099538104321,
          1099540725761, 1099540856833, 1099543085057, 1099544002561]
GATE_P = [3298535669761]
GATES = {"and": lambda a, b: a & b, "or": lambda a, b: a | b, "xor": lambda a, b: a ^ b, "nand": lambda a, b: 1 - (a & b),
         "nor": lambda a, b: 1 - (a | b), "xnor": lambda a, b: 1 - (a ^ b)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_context(hg, name):
    if name == "bit":
        c = hg.Context.from_bit_sizes(hg.CKKS, N, [42] + [41] * 17, [60], sec=hg.SEC_NONE)
    elif name == "gate":
        c = hg.Context.from_primes(hg.CKKS, N, GATE_Q + GATE_P, len(GATE_Q), len(GATE_P))
    else:
        c = hg.Context.from_bit_sizes(hg.CKKS, N, *CHAINS[name], sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    c.upload()
    return c, primes


def chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, cs, ct2, cs2, batch):
    """the refresh entry by entry, every intermediate in a buffer of its own; returns the result, its item stride and the
    raised ciphertext with its stride"""
    Q = c.Q_size
    new = lambda words: torch.full((words,), SENT, dtype=torch.int64, device="cuda")  # noqa: E731
    ws_of = lambda nbytes: torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device="cuda")  # noqa: E731
    limbs = plan.in_level + 1
    words = 2 * limbs * N
    cur, stride = ct, cs
    if ct2 is not None:
        cur, stride = new(batch * words), words
        for b in range(batch):
            c.addition(ct[b * cs:b * cs + words].clone(), ct2[b * cs2:b * cs2 + words].clone(), cur[b * words:(b + 1) * words],
                       limbs, 2, 1, op=0)

    def transforms(cur, stride, factors, depth):
        for k, (diags, n_diag, index, bk, be, gk, ge) in enumerate(factors):
            d = depth + k
            out_words = 2 * (Q - d) * N
            dst = new(batch * out_words)
            c.ckks_linear_transform(cur, stride, dst, out_words, diags, n_diag, index, bk, be, gk, ge, d, batch,
                                    ws_of(c.linear_transform_workspace_bytes(len(be), len(ge), d, batch)))
            c.ckks_rescale_inplace(dst, out_words, d, batch, c.workspace(hg.OP_CKKS_RESCALE, d, batch))
            cur, stride = dst, out_words
        return cur, stride

    cur, stride = transforms(cur, stride, stc, Q - 1 - plan.in_level)
    raise_depth = Q - 1 - plan.cts_level
    rs = 2 * (plan.cts_level + 1) * N
    raised = new(batch * rs)
    c.ckks_mod_raise(cur, stride, raised, rs, raise_depth, batch, c.workspace(hg.OP_CKKS_MOD_RAISE, raise_depth, batch))
    cur, stride = transforms(raised, rs, cts, raise_depth)
    d = raise_depth + plan.cts_pieces
    conj = new(batch * stride)
    c.ckks_apply_galois(cur, stride, conj, stride, keys["conj"], 2 * N - 1, d, batch, c.workspace(hg.OP_CKKS_GALOIS, d, batch))
    hs = 2 * (plan.eval_level + 1) * N
    real = new(batch * hs)
    c.ckks_conj_real(cur, stride, conj, stride, real, hs, d, d + 1, batch)
    trig = plan.trig
    es = 2 * trig.out_limbs * N
    out = new(batch * es)
    depth = Q - 1 - plan.eval_level
    c.ckks_poly_eval(real, hs, out, es, trig, keys["relin"], depth, batch, ws_of(c.poly_eval_workspace_bytes(trig, depth, batch)))
    return out, es, raised, rs


# ---------------------------------------------------------------- 1. the entry against the chain of single entries
_synthetic = {}


def synthetic(hg, name, function):
    """context, plan, synthetic factors and keys of one chain (kept for the module)"""
    if (name, function) in _synthetic:
        return _synthetic[(name, function)]
    if name not in _synthetic:
        c, primes = make_context(hg, name)
        key = lambda seed: hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, seed))  # noqa: E731
        _synthetic[name] = (c, primes, [key(11), key(12), key(13)], {"conj": key(20), "relin": key(21)})
    c, primes, pool, keys = _synthetic[name]
    plan = hg.slim_bootstrap_plan(primes[:c.Q_size], 2.0 ** 40, c.Q_size - 1, function)
    seed = [0]

    def encode(values, scale, limbs):  # residues in place of an encoded diagonal
        seed[0] += 1
        return hg.to_device(synth_ct(primes, range(limbs), 1, N, 7000 + seed[0]))
    cts, stc, elts = c.slim_bootstrap_factors(plan, lambda e: pool[e % 3], encode)
    _synthetic[(name, function)] = (c, primes, plan, cts, stc, keys)
    return _synthetic[(name, function)]


CASES = [(name, function, batch) for name in CHAINS for function in ("slim", "and") for batch in (1, 2)]


@pytest.mark.parametrize("name,function,batch", CASES)
def test_entry_equals_the_chain_of_single_entries(hg, torch, name, function, batch):
    c, primes, plan, cts, stc, keys = synthetic(hg, name, function)
    assert (plan.in_level, plan.cts_level, plan.eval_level, plan.out_level) == (3, 17, 13, 5)
    assert plan.out_scale == (plan.eval_out_scale / 256.0 if function == "slim" else plan.eval_out_scale)
    words = 2 * 4 * N
    cs, cs2 = words + N, words + 3 * N  # N and 3 N words of padding between the items
    cbuf, cbuf2 = np.full(batch * cs, SENT, dtype=np.uint64), np.full(batch * cs2, SENT, dtype=np.uint64)
    for b in range(batch):  # distinct items
        cbuf[b * cs:b * cs + words] = synth_ct(primes, range(4), 2, N, 900 + b)
        cbuf2[b * cs2:b * cs2 + words] = synth_ct(primes, range(4), 2, N, 950 + b)
    ct = hg.to_device(cbuf)
    ct2 = hg.to_device(cbuf2) if function == "and" else None
    ow = 2 * (plan.out_level + 1) * N
    assert plan.trig.out_limbs == plan.out_level + 1  # a double-angle step ends the plan: no rescale after it
    so = ow + N
    out = torch.full((batch * so,), SENT, dtype=torch.int64, device="cuda")
    need = c.slim_bootstrap_workspace_bytes(plan, cts, stc, batch)
    assert need > 0 and c.workspace_bytes(28, 0, batch) == 0
    ws = torch.full((need // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    c.ckks_slim_bootstrap(ct, cs, out, so, plan, cts, stc, keys["conj"], keys["relin"], batch, ws[:need // 8], ct2=ct2, cs2=cs2)
    torch.cuda.synchronize()
    want, ws_stride, _, _ = chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, cs, ct2, cs2, batch)
    torch.cuda.synchronize()
    g, w = hg.to_host(out).reshape(batch, so), hg.to_host(want).reshape(batch, ws_stride)
    assert np.array_equal(g[:, :ow], w[:, :ow]), (name, function, batch)
    assert batch == 1 or not np.array_equal(g[0, :ow], g[1, :ow])
    assert np.all(g[:, ow:] == SENT), "the padding between the items is untouched"
    assert np.array_equal(hg.to_host(ct), cbuf), "the input is not written"
    assert ct2 is None or np.array_equal(hg.to_host(ct2), cbuf2), "the second input is not written"
    assert int(hg.to_host(ws[need // 8:])[0]) == SENT, "the word behind the workspace is intact"


# ---------------------------------------------------------------- 2. encrypted accuracy
_real = {}


def real(hg, name, scale, function):
    """context, plan, keys from a seeded Rng (a secret of weight 32) and the encoded factors (kept for the module).  The
    factors depend on the function through its ratio alone, so the six gates share theirs."""
    if name not in _real:
        c, primes = make_context(hg, name)
        rng = hg.Rng(2027)
        sk = c.generate_secret_key(rng, 32)
        pk = c.generate_public_key(rng, sk)
        keys = {"relin": c.generate_relin_key(rng, sk)}
        galois = {}

        def galois_key(e):
            if e not in galois:
                galois[e] = c.generate_galois_key(rng, sk, e)
            return galois[e]
        plan = hg.slim_bootstrap_plan(primes[:c.Q_size], scale, c.Q_size - 1, function)
        cts, stc, elts = c.slim_bootstrap_factors(plan, galois_key)
        keys["conj"] = galois_key(2 * N - 1)
        assert sorted(galois) == elts
        _real[name] = (c, primes, rng, sk, pk, keys, cts, stc, plan)
    c, primes, rng, sk, pk, keys, cts, stc, first = _real[name]
    plan = hg.slim_bootstrap_plan(primes[:c.Q_size], scale, c.Q_size - 1, function)
    assert plan.stc_scale == first.stc_scale and plan.cts_scale == first.cts_scale
    return c, primes, rng, sk, pk, keys, cts, stc, plan


def encrypt_slots(c, torch, rng, pk, values, scale, limbs):
    """encode real slot values, encrypt, keep the first `limbs` limbs of both parts"""
    z = torch.from_numpy(np.asarray(values, dtype=np.complex128)).cuda()
    full = c.ckks_encrypt(rng, pk, c.ckks_encode_ex(1, z, scale))
    Q = c.Q_size
    return torch.cat([full[:limbs * N], full[Q * N:Q * N + limbs * N]]).contiguous()


def refresh(hg, torch, c, sk, plan, keys, cts, stc, ct, ct2=None):
    words = 2 * (plan.in_level + 1) * N
    room = 2 * plan.trig.out_limbs * N
    out = torch.empty(room, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.slim_bootstrap_workspace_bytes(plan, cts, stc, 1) // 8, dtype=torch.int64, device="cuda")
    c.ckks_slim_bootstrap(ct, words, out, room, plan, cts, stc, keys["conj"], keys["relin"], 1, ws, ct2=ct2, cs2=words)
    depth = c.Q_size - 1 - plan.out_level
    return c.ckks_decode_ex(1, c.ckks_decrypt(out, sk, depth=depth), plan.out_scale, depth=depth).cpu().numpy()


def precondition(hg, torch, c, primes, sk, plan, cts, stc, keys, ct, ct2, tag):
    words = 2 * (plan.in_level + 1) * N
    _, _, raised, _ = chain_of_single_entries(hg, torch, c, plan, cts, stc, keys, ct, words, ct2, words, 1)
    I, t = overflow_of_the_raise(hg, torch, c, primes, sk, raised, c.Q_size - 1 - plan.cts_level)
    worst = np.abs(t).max() / primes[0]
    print(f"{tag}: max |I| = {np.abs(I).max()} (K = {K}), deviation {I.std():.2f}, max |t| / q_0 = {worst:.2f}")
    assert np.abs(I).max() < K and worst < K, "an overflow of the raise outside the range the polynomial is built for"


def eight_values():
    z = np.zeros(SLOTS)
    z[:8] = np.array([1.00, -0.50, 0.25, -1.75, 2.50, -3.25, 0.125, -0.875]) / 8
    return z


@pytest.mark.parametrize("which", ["eight_values", "random_all_slots"])
def test_slim_refreshed_slots(hg, torch, which):
    scale, rho = 2.0 ** 40, 256.0
    c, primes, rng, sk, pk, keys, cts, stc, plan = real(hg, "A", scale, "slim")
    z = eight_values() if which == "eight_values" else np.random.default_rng(5).uniform(-0.5, 0.5, SLOTS)
    ct = encrypt_slots(c, torch, rng, pk, z, scale, plan.in_level + 1)
    precondition(hg, torch, c, primes, sk, plan, cts, stc, keys, ct, None, f"slim {which}")
    got = refresh(hg, torch, c, sk, plan, keys, cts, stc, ct)
    f = rho / (2 * np.pi) * np.sin(2 * np.pi * z / rho)
    err = np.abs(got - f).max()
    print(f"slim {which}: max |refreshed - f(z)| = {err:.3e} over {SLOTS} slots (criterion 1e-4); against z itself "
          f"{np.abs(got - z).max():.3e}; largest imaginary part {np.abs(got.imag).max():.3e}")
    assert plan.out_level == 5 and abs(plan.out_scale * rho / primes[plan.eval_level] - 1) <= 1e-12
    assert err < 1e-4


def test_bit_refreshed_slots(hg, torch):
    scale = 2.0 ** 41
    c, primes, rng, sk, pk, keys, cts, stc, plan = real(hg, "bit", scale, "bit")
    g = np.random.default_rng(7)
    b = g.integers(0, 2, SLOTS)
    b[:4] = [0, 0, 1, 1]
    e = g.uniform(-0.02, 0.02, SLOTS)
    e[:4] = [0.02, -0.02, 0.02, -0.02]
    ct = encrypt_slots(c, torch, rng, pk, b + e, scale, plan.in_level + 1)
    precondition(hg, torch, c, primes, sk, plan, cts, stc, keys, ct, None, "bit")
    got = refresh(hg, torch, c, sk, plan, keys, cts, stc, ct)
    err = np.abs(got - b).max()
    clean = np.abs(got - (0.5 - 0.5 * np.cos(np.pi * (b + e)))).max()
    bound = (np.pi * 0.02) ** 2 / 4 + 1e-4
    print(f"bit: max |refreshed - b| = {err:.3e} over {SLOTS} slots (bound {bound:.3e}, the input's own error 2.0e-02); "
          f"against 1/2 - 1/2 cos(pi (b + e)) {clean:.3e}")
    assert err <= bound


@pytest.mark.parametrize("gate", sorted(GATES))
def test_gate_refreshed_slots(hg, torch, gate):
    scale = 2.0 ** 40
    c, primes, rng, sk, pk, keys, cts, stc, plan = real(hg, "gate", scale, gate)
    a, b = (np.arange(SLOTS) >> 1) & 1, np.arange(SLOTS) & 1  # (0,0) (0,1) (1,0) (1,1) over and over
    if "inputs" not in _real:
        _real["inputs"] = (encrypt_slots(c, torch, rng, pk, a, scale, plan.in_level + 1),
                           encrypt_slots(c, torch, rng, pk, b, scale, plan.in_level + 1))
        precondition(hg, torch, c, primes, sk, plan, cts, stc, keys, *_real["inputs"], "gates")
    ct, ct2 = _real["inputs"]
    got = refresh(hg, torch, c, sk, plan, keys, cts, stc, ct, ct2)
    want = GATES[gate](a, b)
    err = np.abs(got - want).max()
    print(f"{gate}: max |refreshed - gate(a, b)| = {err:.3e} over {SLOTS} slots (criterion 1e-4)")
    assert np.array_equal(np.rint(got.real).astype(np.int64), want), "a wrong bit"
    assert err < 1e-4


# ---------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(hg, torch):
    c, primes, plan, cts, stc, keys = synthetic(hg, "A", "and")
    Q = c.Q_size
    words = 2 * 4 * N
    ct = hg.to_device(synth_ct(primes, range(4), 2, N, 1))
    ct2 = hg.to_device(synth_ct(primes, range(4), 2, N, 2))
    room = 2 * plan.trig.out_limbs * N
    buf = torch.full((2 * room,), SENT, dtype=torch.int64, device="cuda")
    out = buf[:room]
    ws = torch.full((c.slim_bootstrap_workspace_bytes(plan, cts, stc, 1) // 8,), SENT, dtype=torch.int64, device="cuda")

    def refused(fn):
        with pytest.raises(hg.HEError) as e:
            fn()
        assert e.value.code == hg.E_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote its result buffer"
        assert bool((ws == SENT).all()), "a refused call wrote its workspace"

    call = lambda **kw: c.ckks_slim_bootstrap(kw.pop("ct", ct), words, kw.pop("out", out), room, kw.pop("plan", plan),  # noqa: E731
                                              kw.pop("cts", cts), kw.pop("stc", stc), keys["conj"], keys["relin"],
                                              kw.pop("batch", 1), kw.pop("ws", ws), ct2=kw.pop("ct2", ct2), cs2=words)
    refused(lambda: call(batch=0))
    refused(lambda: call(ws=ws[:ws.numel() - 1]))
    # a plan that does not fit the context (made for a chain one limb longer), a factor list of the wrong length
    refused(lambda: call(plan=hg.slim_bootstrap_plan(primes[:Q] + [primes[Q - 1]], 2.0 ** 40, Q, "and")))
    refused(lambda: call(cts=cts[:2]))
    refused(lambda: call(stc=stc + stc[:1]))
    # a plan whose polynomial is another plan's
    other = hg.eval_trig_plan(K, 30, 3, plan.phase, plan.amplitude, plan.offset, plan.eval_level, plan.eval_in_scale, 2.0 ** 49, primes[:Q])
    refused(lambda: call(plan=hg.SlimBootstrapPlan(plan.c, other)))
    # an output overlapping an input or the workspace, the second input inside the workspace
    joint = torch.full((words + room,), SENT, dtype=torch.int64, device="cuda")
    refused(lambda: call(ct=joint[:words], out=joint[words - 1:words - 1 + room]))
    refused(lambda: call(ct2=joint[:words], out=joint[words - 1:words - 1 + room]))
    refused(lambda: call(out=ws[:room]))
    refused(lambda: call(ct2=ws[:words]))
    torch.cuda.synchronize()
    assert bool((joint == SENT).all())
