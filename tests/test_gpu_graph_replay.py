"""Every operator family on a side stream and from a captured graph (helpers.side_stream_and_graph_parity).

include/hegpu.h promises that an entry with a `stream` argument issues all its work on that stream, allocates nothing and
does not synchronise, so that a caller may record it into a hipGraph.  Every other GPU test calls on the null stream, where
a launch that forgot its stream, a memset on stream 0 or a function-attribute static that first runs inside the call is
still serialised and passes.  Here each family runs (1) eagerly on a side stream while the null stream is busy, and (2)
captured once on that side stream and replayed on two fresh inputs, outputs and workspaces holding a poison word before
every run.  Results are the CPU oracle's bit for bit; where the oracle has no entry, the chain of single entries run
eagerly on the same inputs (each docstring names the test that pins that chain).

N = 4096 (the smallest degree the transforms accept) unless a test says otherwise, batch 2, the items of every operand one
word further apart than they are long.

The second half: entries that draw randomness or synchronise refuse a capturing stream with HEGPU_E_LOGIC before anything
is queued and before the generator's counter moves."""
import numpy as np
import pytest

from helpers import side_stream_and_graph_parity as parity
from helpers import synth_ct, synth_key

pytestmark = pytest.mark.gpu

N = 4096
B = 2
SEEDS = (3, 8)  # the two replayed inputs; the warm-up runs on zeros


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def zeros(words, count=B, dtype=np.uint64):
    return [np.zeros(words, dtype=dtype) for _ in range(count)]


def ws_of(nbytes):
    """a workspace operand of exactly nbytes bytes"""
    return ([np.zeros(max(nbytes // 8, 1), dtype=np.uint64)], "ws")


_made = {}


def ckks(hg, oracle, log_q, log_p, n=N):
    tag = ("ckks", tuple(log_q), tuple(log_p), n)
    if tag not in _made:
        c = hg.Context.from_bit_sizes(hg.CKKS, n, list(log_q), list(log_p), sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
        c.upload()
        _made[tag] = (c, o, primes)
    return _made[tag]


def bfv(hg, oracle):
    if "bfv" not in _made:
        t = 1032193
        c = hg.Context.from_default(hg.BFV, N, 1, t)
        primes = [int(x) for x in c.table("modulus")]
        o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, t)
        c.upload()
        _made["bfv"] = (c, o, primes, t)
    return _made["bfv"]


def packed(hg, items):
    """the items of a batch as one contiguous device tensor: what the chains of single entries take"""
    return hg.to_device(np.concatenate(items))


def with_options(c, options, fn):
    try:
        for k, v in options.items():
            c.set_option(k, v)
        fn()
    finally:
        for k in options:
            c.set_option(k, -1)


# ------------------------------------------------------------------ CKKS, key-switch method II
@pytest.mark.parametrize("form", ["by_launch_size", "forced_fused"])
def test_ckks_method_II_sequence(hg, oracle, torch, form):
    """multiply -> relinearize_inplace -> rescale_inplace -> apply_galois at depth 1 of {60, 45, 45, 45 | 60, 50}, the
    launch forms chosen by launch size and with fused_row_mac = 1, col_multi = 1: the oracle's residues"""
    c, o, primes = ckks(hg, oracle, [60, 45, 45, 45], [60, 50])
    Q, Qp, depth = c.Q_size, c.Q_prime_size, 1
    l, digits = Q - depth, c.switch_key_digits()
    assert c.P_size == 2 and digits == 2
    key, gkey = synth_key(primes, digits, Qp, N, 3), synth_key(primes, digits, Qp, N, 4)
    gal = hg.steps_to_galois_elt(1, N, 5)

    def case(seed):
        ct1 = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        ct2 = [synth_ct(primes, range(l), 2, N, seed + 10 * b + 1) for b in range(B)]
        out, rot = [], []
        for b in range(B):
            w = o.ckks_relinearize_II(o.ckks_multiply(ct1[b], ct2[b], depth), key, depth)
            r = o.ckks_rescale(w[:2 * l * N].copy(), depth)[:2 * (l - 1) * N]
            out.append(r)
            rot.append(o.ckks_apply_galois_II(r, gkey, gal, depth + 1))
        return {"ct1": ct1, "ct2": ct2}, {"out": out, "rot": rot}

    operands = {"ct1": (zeros(2 * l * N), "in"), "ct2": (zeros(2 * l * N), "in"), "out": (zeros(3 * l * N), "out"),
                "rot": (zeros(2 * (l - 1) * N), "out"), "key": ([key], "in"), "gkey": ([gkey], "in"),
                "ws_relin": ws_of(c.workspace_bytes(hg.OP_CKKS_RELIN, depth, B)),
                "ws_resc": ws_of(c.workspace_bytes(hg.OP_CKKS_RESCALE, depth, B)),
                "ws_gal": ws_of(c.workspace_bytes(hg.OP_CKKS_GALOIS, depth + 1, B))}

    def call(d, s):
        c.ckks_multiply(d["ct1"], s["ct1"], d["ct2"], s["ct2"], d["out"], s["out"], depth, B)
        c.ckks_relinearize_inplace(d["out"], s["out"], d["key"], depth, B, d["ws_relin"])
        c.ckks_rescale_inplace(d["out"], s["out"], depth, B, d["ws_resc"])
        c.ckks_apply_galois(d["out"], s["out"], d["rot"], s["rot"], d["gkey"], gal, depth + 1, B, d["ws_gal"])

    cases = [case(seed) for seed in SEEDS]
    options = dict(fused_row_mac=1, col_multi=1) if form == "forced_fused" else {}
    with_options(c, options, lambda: parity(torch, operands, call, cases))


# ------------------------------------------------------------------ hoisted rotations
def test_hoisted_rotations(hg, oracle, torch):
    """ckks_rotate_hoisted, five elements with the identity 0 and the conjugation 2N - 1 among them, on the
    four-accumulator workspace (OP_CKKS_ROTATE_HOISTED), depth 1 of {60, 40, 45, 40 | 60}: the oracle's residues"""
    c, o, primes = ckks(hg, oracle, [60, 40, 45, 40], [60])
    Q, Qp, depth = c.Q_size, c.Q_prime_size, 1
    l = Q - depth
    words = 2 * l * N
    elts = [0, hg.steps_to_galois_elt(1, N, 5), hg.steps_to_galois_elt(-2, N, 5), 2 * N - 1, hg.steps_to_galois_elt(5, N, 5)]
    keys = [None if g == 0 else synth_key(primes, c.switch_key_digits(), Qp, N, 20 + i) for i, g in enumerate(elts)]

    def case(seed):
        cts = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        return {"ct": cts}, {"out": [o.ckks_rotate_hoisted(x, keys, elts, depth) for x in cts]}

    operands = {"ct": (zeros(words), "in"), "out": (zeros(len(elts) * words), "out"),
                "ws": ws_of(c.workspace_bytes(hg.OP_CKKS_ROTATE_HOISTED, depth, B))}
    for i, k in enumerate(keys):
        if k is not None:
            operands["key%d" % i] = ([k], "in")
    call = lambda d, s: c.ckks_rotate_hoisted(d["ct"], s["ct"], d["out"], s["out"],  # noqa: E731
                                              [d.get("key%d" % i) for i in range(len(elts))], elts, depth, B, d["ws"])
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ BFV
@pytest.mark.parametrize("behz_split", [0, 1])
def test_bfv_sequence(hg, oracle, torch, behz_split):
    """bfv_multiply (both BEHZ launch forms) -> bfv_relinearize_inplace -> bfv_apply_galois, and bfv_multiply_plain of the
    first input, on the default chain with t = 1032193: the oracle's residues"""
    c, o, primes, t = bfv(hg, oracle)
    Q, Qp = c.Q_size, c.Q_prime_size
    words = 2 * Q * N
    key, gkey = synth_key(primes, c.switch_key_digits(), Qp, N, 3), synth_key(primes, c.switch_key_digits(), Qp, N, 4)
    g = hg.steps_to_galois_elt(1, N, 3)
    mp_bytes = c.workspace_bytes(hg.OP_BFV_MULTIPLY_PLAIN, 0, 1)

    def case(seed):
        ct1 = [synth_ct(primes, range(Q), 2, N, seed + 10 * b) for b in range(B)]
        ct2 = [synth_ct(primes, range(Q), 2, N, seed + 10 * b + 1) for b in range(B)]
        plain = [np.random.default_rng(seed + b).integers(0, t, N).astype(np.uint64) for b in range(B)]
        for p in plain:
            p[:4] = [0, t - 1, (t + 1) // 2, (t + 1) // 2 - 1]
        out, rot, mp = [], [], []
        for b in range(B):
            w = o.bfv_relinearize(o.bfv_multiply(ct1[b], ct2[b]), key)[:words]
            out.append(w)
            rot.append(o.bfv_apply_galois(w, gkey, g))
            mp.append(o.bfv_multiply_plain(ct1[b], plain[b]))
        return {"ct1": ct1, "ct2": ct2, "plain": plain}, {"out": out, "rot": rot, "mp": mp}

    operands = {"ct1": (zeros(words), "in"), "ct2": (zeros(words), "in"), "plain": (zeros(N), "in"),
                "out": (zeros(3 * Q * N), "out"), "rot": (zeros(words), "out"), "mp": (zeros(words), "out"),
                "key": ([key], "in"), "gkey": ([gkey], "in"),
                "ws_mul": ws_of(c.workspace_bytes(hg.OP_BFV_MULTIPLY, 0, B)),
                "ws_relin": ws_of(c.workspace_bytes(hg.OP_BFV_RELIN, 0, B)),
                "ws_gal": ws_of(c.workspace_bytes(hg.OP_BFV_GALOIS, 0, B)), "ws_mp": ws_of(mp_bytes)}

    def call(d, s):
        c.bfv_multiply(d["ct1"], s["ct1"], d["ct2"], s["ct2"], d["out"], s["out"], B, d["ws_mul"])
        c.bfv_relinearize_inplace(d["out"], s["out"], d["key"], B, d["ws_relin"])
        c.bfv_apply_galois(d["out"], s["out"], d["rot"], s["rot"], d["gkey"], g, B, d["ws_gal"])
        for b in range(B):  # one item per call
            c._call("bfv_multiply_plain", d["ct1"][b * s["ct1"]:].data_ptr(), d["plain"][b * s["plain"]:].data_ptr(),
                    d["mp"][b * s["mp"]:].data_ptr(), d["ws_mp"].data_ptr(), mp_bytes)

    cases = [case(seed) for seed in SEEDS]
    with_options(c, dict(behz_split=behz_split), lambda: parity(torch, operands, call, cases))


# ------------------------------------------------------------------ linear transform
def test_diag_mac(hg, torch):
    """ckks_diag_mac, n1 = 4, n2 = 3, rows with absent (-1) diagonals, 60-bit moduli: the Python-integer model of
    tests/test_gpu_linear_transform.py"""
    from test_gpu_linear_transform import _want_diag_mac
    from test_gpu_poly_eval import context
    c, primes = context(hg, [60, 60, 60], [60])
    l, n1, n2, n_diag = 3, 4, 3, 8
    index = [[0, 1, 2, 3], [4, -1, 5, -1], [-1, 6, -1, 7]]
    words = 2 * l * N
    diags = np.stack([synth_ct(primes, range(l), 1, N, 900 + k).reshape(l, N) for k in range(n_diag)])

    def case(seed):
        rot = [np.stack([synth_ct(primes, range(l), 2, N, seed + 100 * b + i).reshape(2, l, N) for i in range(n1)]) for b in range(B)]
        want = [_want_diag_mac(rot[b], diags, index, primes, l).reshape(-1) for b in range(B)]
        return {"rot": [r.reshape(-1) for r in rot]}, {"out": want}

    operands = {"rot": (zeros(n1 * words), "in"), "diags": ([diags.reshape(-1)], "in"), "out": (zeros(n2 * words), "out")}
    call = lambda d, s: c.ckks_diag_mac(d["rot"], s["rot"], n1, d["diags"], n_diag, index, n2, d["out"], s["out"], 0, B)  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_linear_transform(hg, torch):
    """ckks_linear_transform, seven diagonals with n1 = 4, n2 = 3, absent (-1) index entries and the giant element 0: the
    composition of single entries (rotate_hoisted, cipherplain_multiplication, addition, apply_galois) that
    test_gpu_linear_transform.py::test_fused_entry_equals_the_composition pins the entry to"""
    from test_gpu_linear_transform import SLOTS, _composition, _key, _set
    entry = _set(hg, "method_I")
    c, primes, _ = entry
    depth = 0
    l = c.Q_size - depth
    words = 2 * l * N
    ks = [0, 1, 2, 3, 5, 8, 9]
    plan = hg.linear_transform_plan(ks, SLOTS, 4)
    assert (plan.n1, plan.n2) == (4, 3) and plan.giant_shifts[0] == 0 and any(v < 0 for row in plan.index for v in row)
    n_diag = len(ks)
    host_diags = np.concatenate([synth_ct(primes, range(l), 1, N, 600 + k) for k in range(n_diag)])
    diags = hg.to_device(host_diags).reshape(n_diag, l * N)
    belts = [hg.steps_to_galois_elt(sh, N, 5) if sh else 0 for sh in plan.baby_shifts]
    gelts = [hg.steps_to_galois_elt(sh, N, 5) if sh else 0 for sh in plan.giant_shifts]
    bkeys = [_key(hg, entry, sh) if sh else None for sh in plan.baby_shifts]
    gkeys = [_key(hg, entry, sh) if sh else None for sh in plan.giant_shifts]

    def case(seed):
        cts = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        want = _composition(hg, torch, c, packed(hg, cts), words, diags, plan, bkeys, belts, gkeys, gelts, depth, B)
        return {"ct": cts}, {"out": list(want)}

    operands = {"ct": (zeros(words), "in"), "diags": ([host_diags], "in"), "out": (zeros(words), "out"),
                "ws": ws_of(c.linear_transform_workspace_bytes(plan.n1, plan.n2, depth, B))}
    call = lambda d, s: c.ckks_linear_transform(d["ct"], s["ct"], d["out"], s["out"], d["diags"], n_diag, plan.index,  # noqa: E731
                                                bkeys, belts, gkeys, gelts, depth, B, d["ws"])
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ CoeffToSlot / SlotToCoeff and their boundary passes
def _transform_setup(hg):
    """the context, conjugation key and synthetic factors of tests/test_gpu_encoding_transform.py, method I, two factors
    each way (the smallest count that module builds)"""
    if "transform" not in _made:
        from test_gpu_encoding_transform import SETS, _synthetic_factors
        c = hg.Context.from_bit_sizes(hg.CKKS, N, *SETS["method_I"], sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        c.upload()
        keys = {}
        conj = hg.to_device(synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 5))
        cts = _synthetic_factors(hg, c, primes, True, 2, 1, keys)
        stc = _synthetic_factors(hg, c, primes, False, 2, 3, keys)
        _made["transform"] = (c, primes, conj, cts, stc)
    return _made["transform"]


def test_coeff_to_slot(hg, torch):
    """ckks_coeff_to_slot from depth 1, two factors: the chain linear_transform + rescale_inplace per factor, apply_galois
    with 2N - 1 and conj_split, as in test_gpu_encoding_transform.py::test_sequences_equal_the_chain_of_single_entries"""
    from test_gpu_encoding_transform import _chain
    c, primes, conj, factors, _ = _transform_setup(hg)
    Q, P, depth = c.Q_size, 2, 1
    l = Q - depth
    t_stride, ow = 2 * l * N, 2 * (l - P - 1) * N
    args = [a for a, _ in factors]

    def case(seed):
        cts = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        x = _chain(hg, torch, c, packed(hg, cts), t_stride, factors, depth, B, t_stride)
        xc = torch.empty_like(x)
        c.ckks_apply_galois(x, t_stride, xc, t_stride, conj, 2 * N - 1, depth + P, B, c.workspace(hg.OP_CKKS_GALOIS, depth + P, B))
        w0, w1 = torch.empty(B * ow, dtype=torch.int64, device="cuda"), torch.empty(B * ow, dtype=torch.int64, device="cuda")
        c.ckks_conj_split(x, t_stride, xc, t_stride, w0, w1, ow, depth + P, depth + P + 1, B)
        torch.cuda.synchronize()
        return {"ct": cts}, {"out0": list(hg.to_host(w0).reshape(B, ow)), "out1": list(hg.to_host(w1).reshape(B, ow))}

    operands = {"ct": (zeros(t_stride), "in"), "out0": (zeros(ow), "out"), "out1": (zeros(ow), "out"),
                "ws": ws_of(c.encoding_transform_workspace_bytes(args, depth, B))}
    call = lambda d, s: c.ckks_coeff_to_slot(d["ct"], s["ct"], d["out0"], d["out1"], s["out0"], args, conj, depth, B, d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_slot_to_coeff(hg, torch):
    """ckks_slot_to_coeff from depth 2, two factors: conj_merge, then linear_transform + rescale_inplace per factor, as in
    test_gpu_encoding_transform.py::test_sequences_equal_the_chain_of_single_entries"""
    from test_gpu_encoding_transform import _chain
    c, primes, conj, _, factors = _transform_setup(hg)
    Q, P, depth = c.Q_size, 2, 2
    l = Q - depth
    in_words, room, ow, t_stride = 2 * l * N, 2 * (l - P) * N, 2 * (l - P - 1) * N, 2 * (l - 1) * N
    args = [a for a, _ in factors]

    def case(seed):
        c0 = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        c1 = [synth_ct(primes, range(l), 2, N, seed + 10 * b + 5) for b in range(B)]
        merged = torch.empty(B * t_stride, dtype=torch.int64, device="cuda")
        c.ckks_conj_merge(packed(hg, c0), in_words, packed(hg, c1), in_words, merged, t_stride, depth, depth + 1, B)
        want = _chain(hg, torch, c, merged, t_stride, factors, depth + 1, B, t_stride)
        torch.cuda.synchronize()
        return {"c0": c0, "c1": c1}, {"out": [w[:ow] for w in hg.to_host(want).reshape(B, t_stride)]}

    operands = {"c0": (zeros(in_words), "in"), "c1": (zeros(in_words), "in"), "out": (zeros(room), "out"),
                "ws": ws_of(c.encoding_transform_workspace_bytes(args, depth, B))}
    call = lambda d, s: c.ckks_slot_to_coeff(d["c0"], s["c0"], d["c1"], s["c1"], d["out"], s["out"], args, depth, B, d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_conj_split_merge_and_real(hg, torch):
    """ckks_conj_split, ckks_conj_merge and ckks_conj_real, three 60-bit limbs of which one is dropped: the composition of
    hegpu_addition and hegpu_ckks_mult_i of test_gpu_encoding_transform.py::test_conj_split_and_merge_equal_the_composition
    (conj_real is conj_split's first output, tests/test_gpu_conj_real.py)"""
    from test_gpu_poly_eval import context
    c, primes = context(hg, [60, 60, 60], [60])
    Q, l, dropped = c.Q_size, 3, 1
    depth, out_depth, lo = Q - l, Q - l + dropped, l - dropped
    ow = 2 * lo * N

    def case(seed):
        xs = [synth_ct(primes, range(l), 2, N, seed + 10 * b) for b in range(B)]
        ys = [synth_ct(primes, range(l), 2, N, seed + 10 * b + 5) for b in range(B)]
        want = {"out0": [], "out1": [], "merged": [], "real": []}
        for b in range(B):
            a = hg.to_device(np.ascontiguousarray(xs[b].reshape(2, l, N)[:, :lo]).reshape(-1))
            k = hg.to_device(np.ascontiguousarray(ys[b].reshape(2, l, N)[:, :lo]).reshape(-1))
            s_, d_, m = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
            c.addition(a, k, s_, lo, 2, 1, op=0)
            c.addition(a, k, d_, lo, 2, 1, op=1)
            d_ = c.ckks_mult_i(d_, lo, 2, divide=True)
            c.addition(a, c.ckks_mult_i(k, lo, 2, divide=False), m, lo, 2, 1, op=0)
            torch.cuda.synchronize()
            for name, t in (("out0", s_), ("out1", d_), ("merged", m), ("real", s_)):
                want[name].append(hg.to_host(t).copy())
        return {"x": xs, "y": ys}, want

    operands = {"x": (zeros(2 * l * N), "in"), "y": (zeros(2 * l * N), "in"), "out0": (zeros(ow), "out"),
                "out1": (zeros(ow), "out"), "merged": (zeros(ow), "out"), "real": (zeros(ow), "out")}

    def call(d, s):
        c.ckks_conj_split(d["x"], s["x"], d["y"], s["y"], d["out0"], d["out1"], s["out0"], depth, out_depth, B)
        c.ckks_conj_merge(d["x"], s["x"], d["y"], s["y"], d["merged"], s["merged"], depth, out_depth, B)
        c.ckks_conj_real(d["x"], s["x"], d["y"], s["y"], d["real"], s["real"], depth, out_depth, B)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ polynomial evaluation
def test_weighted_sum(hg, torch):
    """ckks_weighted_sum, three terms at 3, 5 and 3 limbs with complex weights: the Python-integer model of
    tests/test_gpu_poly_eval.py"""
    from test_gpu_poly_eval import context, weighted_sum_model
    c, primes = context(hg, [60, 40, 40, 40, 40], [60])
    psi_half = c.table("psi_half")
    limbs, term_limbs = 3, [3, 5, 3]
    g = np.random.default_rng(31)
    weights = [complex(a, b) for a, b in zip(g.integers(-2 ** 40, 2 ** 40, 3), g.integers(-2 ** 40, 2 ** 40, 3))]
    w0 = complex(float(2 ** 80 + 12345 * 2 ** 30), -float(2 ** 41 + 1))

    def case(seed):
        terms = [[synth_ct(primes, range(L), 2, N, seed + 10 * i + b) for b in range(B)] for i, L in enumerate(term_limbs)]
        want = [weighted_sum_model([t[b] for t in terms], term_limbs, weights, w0, limbs, primes, psi_half).reshape(-1)
                for b in range(B)]
        return {"t%d" % i: t for i, t in enumerate(terms)}, {"out": want}

    operands = {"t%d" % i: (zeros(2 * L * N), "in") for i, L in enumerate(term_limbs)}
    operands["out"] = (zeros(2 * limbs * N), "out")
    call = lambda d, s: c.ckks_weighted_sum([d["t%d" % i] for i in range(3)], [s["t%d" % i] for i in range(3)], term_limbs,  # noqa: E731
                                            weights, w0, d["out"], s["out"], limbs, batch=B)
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_double_sub(hg, torch):
    """ckks_double_sub, 2 a - b with a at 4 and b at 5 limbs on 3 limbs: the chain addition(a, a), addition(op 1) of
    test_gpu_poly_eval.py::test_double_sub_equals_its_chain"""
    from test_gpu_poly_eval import context, drop
    c, primes = context(hg, [60, 40, 40, 40, 40], [60])
    limbs, a_limbs, b_limbs = 3, 4, 5
    words = 2 * limbs * N

    def case(seed):
        a = [synth_ct(primes, range(a_limbs), 2, N, seed + b) for b in range(B)]
        b_ct = [synth_ct(primes, range(b_limbs), 2, N, seed + 20 + b) for b in range(B)]
        a2 = drop(packed(hg, a), B, a_limbs, limbs)
        c.addition(a2, a2, a2, limbs, 2, B)
        c.addition(a2, drop(packed(hg, b_ct), B, b_limbs, limbs), a2, limbs, 2, B, op=1)
        torch.cuda.synchronize()
        return {"a": a, "b": b_ct}, {"out": list(hg.to_host(a2).reshape(B, words))}

    operands = {"a": (zeros(2 * a_limbs * N), "in"), "b": (zeros(2 * b_limbs * N), "in"), "out": (zeros(words), "out")}
    call = lambda d, s: c.ckks_double_sub(d["a"], s["a"], a_limbs, d["b"], s["b"], b_limbs, 0.0, d["out"], s["out"], limbs, batch=B)  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_poly_eval(hg, torch):
    """ckks_poly_eval, a degree-7 Chebyshev plan at depth 1, method I: the plan step by step with multiply, relinearize,
    rescale and the additions (compose) of test_gpu_poly_eval.py::test_poly_eval_equals_the_step_by_step_composition"""
    from heongpu_amd import api
    from test_gpu_poly_eval import SETS, compose, context
    c, primes = context(hg, *SETS["method_I"])
    Q, depth = c.Q_size, 1
    l = Q - depth
    coeffs = np.random.default_rng(7).uniform(-1, 1, 8)
    scale = float(primes[1])
    plan = hg.poly_eval_plan(api.CHEBYSHEV, coeffs, Q - 1 - depth, scale, scale, primes[:Q])
    key_host = synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 3)
    key = hg.to_device(key_host)
    words = 2 * (plan.level + 1) * N

    def case(seed):
        cts = [synth_ct(primes, range(l), 2, N, seed + b) for b in range(B)]
        want = compose(c, hg, torch, plan, packed(hg, cts), key, depth, B)
        torch.cuda.synchronize()
        return {"ct": cts}, {"out": list(hg.to_host(want).reshape(B, words))}

    operands = {"ct": (zeros(2 * l * N), "in"), "out": (zeros(2 * plan.out_limbs * N), "out"), "key": ([key_host], "in"),
                "ws": ws_of(c.poly_eval_workspace_bytes(plan, depth, B))}
    call = lambda d, s: c.ckks_poly_eval(d["ct"], s["ct"], d["out"], s["out"], plan, d["key"], depth, B, d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ modulus raise
def test_mod_raise_kernel_and_operator(hg, torch):
    """the kernel entry mod_raise against the integer model `lift` of tests/test_gpu_mod_raise.py, and ckks_mod_raise
    against the chain ntt (inverse) -> mod_raise -> ntt (forward) of that module's ckks_case, {60, 40, 30, 50, 60 | 60}"""
    from test_gpu_mod_raise import context, planted, want_raise
    c, primes = context(hg, "wide_source")
    Q = len(primes)

    def case(seed):
        v = planted(primes, 2, B, N, seed)
        coef = hg.to_device(v.reshape(-1))
        ct = torch.empty_like(coef)
        c.ntt(coef, ct, False, 2 * B, 1)  # the planted values carried to the NTT domain
        back = torch.empty_like(ct)
        c.ntt(ct, back, True, 2 * B, 1)
        raised = torch.empty(B * 2 * Q * N, dtype=torch.int64, device="cuda")
        c.mod_raise(back, 2 * N, raised, 2 * Q * N, Q, 2, B)
        want = torch.empty_like(raised)
        c.ntt(raised, want, False, 2 * Q * B, Q)
        torch.cuda.synchronize()
        return ({"src": list(v.reshape(B, 2 * N)), "ct": list(hg.to_host(ct).reshape(B, 2 * N))},
                {"lifted": list(want_raise(v, primes, Q).reshape(B, 2 * Q * N)), "raised": list(hg.to_host(want).reshape(B, 2 * Q * N))})

    nbytes = c.workspace_bytes(hg.OP_CKKS_MOD_RAISE, 0, B)
    operands = {"src": (zeros(2 * N), "in"), "ct": (zeros(2 * N), "in"), "lifted": (zeros(2 * Q * N), "out"),
                "raised": (zeros(2 * Q * N), "out"), "ws": ws_of(nbytes)}

    def call(d, s):
        c.mod_raise(d["src"], s["src"], d["lifted"], s["lifted"], Q, 2, B)
        c.ckks_mod_raise(d["ct"], s["ct"], d["raised"], s["raised"], 0, B, d["ws"], ws_bytes=nbytes)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ the assembled refreshes
def _eager(torch, hg, run, cts, out_words, ow):
    """the entry on the null stream into buffers of its own: per item the first ow words of the result"""
    out = torch.zeros(B * out_words, dtype=torch.int64, device="cuda")
    run(packed(hg, cts), out)
    torch.cuda.synchronize()
    return [w[:ow] for w in hg.to_host(out).reshape(B, out_words)]


def test_regular_refresh(hg, torch):
    """ckks_bootstrap on chain A of tests/test_gpu_bootstrap.py (synthetic keys and diagonals, no switch keys): the
    replay against the eager call, which test_gpu_bootstrap.py::test_entry_equals_the_chain_of_single_entries pins to
    the chain of single entries"""
    from test_gpu_bootstrap import synthetic
    c, primes, plan, cts, stc, keys = synthetic(hg, "A", 256.0)
    ow, room = 2 * (plan.out_level + 1) * N, 2 * (plan.out_level + 2) * N
    need = c.bootstrap_workspace_bytes(plan, cts, stc, False, B)
    eager_ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")

    def case(seed):
        items = [synth_ct(primes, [0], 2, N, seed + b) for b in range(B)]
        run = lambda ct, out: c.ckks_bootstrap(ct, 2 * N, out, room, plan, cts, stc, keys["conj"], keys["relin"], B, eager_ws)  # noqa: E731
        return {"ct": items}, {"out": _eager(torch, hg, run, items, room, ow)}

    operands = {"ct": (zeros(2 * N), "in"), "out": (zeros(room), "out"), "ws": ws_of(need)}
    call = lambda d, s: c.ckks_bootstrap(d["ct"], s["ct"], d["out"], s["out"], plan, cts, stc, keys["conj"], keys["relin"], B, d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_slim_refresh(hg, torch):
    """ckks_slim_bootstrap on chain A of tests/test_gpu_slim_bootstrap.py (the arithmetic plan, one input): the replay
    against the eager call, which test_gpu_slim_bootstrap.py::test_entry_equals_the_chain_of_single_entries pins to the
    chain of single entries"""
    from test_gpu_slim_bootstrap import synthetic
    c, primes, plan, cts, stc, keys = synthetic(hg, "A", "slim")
    limbs = plan.in_level + 1
    words, ow = 2 * limbs * N, 2 * (plan.out_level + 1) * N
    assert plan.trig.out_limbs == plan.out_level + 1
    need = c.slim_bootstrap_workspace_bytes(plan, cts, stc, B)
    eager_ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")

    def case(seed):
        items = [synth_ct(primes, range(limbs), 2, N, seed + b) for b in range(B)]
        run = lambda ct, out: c.ckks_slim_bootstrap(ct, words, out, ow, plan, cts, stc, keys["conj"], keys["relin"], B, eager_ws)  # noqa: E731
        return {"ct": items}, {"out": _eager(torch, hg, run, items, ow, ow)}

    operands = {"ct": (zeros(words), "in"), "out": (zeros(ow), "out"), "ws": ws_of(need)}
    call = lambda d, s: c.ckks_slim_bootstrap(d["ct"], s["ct"], d["out"], s["out"], plan, cts, stc, keys["conj"], keys["relin"], B, d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ logic gates
@pytest.mark.parametrize("gate,kind", [("AND", "cipher"), ("XOR", "plain")])
def test_ckks_logic_gate(hg, torch, gate, kind):
    """ckks_logic_gate at depth 1, method I: the composition multiply / cipherplain_multiplication, relinearize, rescale
    and the additions of test_gpu_logic.py::test_ckks_logic_gate_equals_its_composition"""
    from test_gpu_logic import CIPHER, PLAIN, SETS, ckks_compose, context, gate_id
    c, primes = context(hg, hg.CKKS, *SETS["method_I"])
    Q, depth = c.Q_size, 1
    l = Q - depth
    k = CIPHER if kind == "cipher" else PLAIN
    b_words = (2 if k == CIPHER else 1) * l * N
    ow = 2 * (l - 1) * N
    key_host = synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 3)
    key = hg.to_device(key_host)
    scale_one = float(primes[1])

    def case(seed):
        a = [synth_ct(primes, range(l), 2, N, seed + i) for i in range(B)]
        b = [synth_ct(primes, range(l), 2 if k == CIPHER else 1, N, seed + 20 + i) for i in range(B)]
        want = ckks_compose(c, hg, torch, gate, packed(hg, a), packed(hg, b), k, key, depth, B, scale_one)
        torch.cuda.synchronize()
        return {"a": a, "b": b}, {"out": list(hg.to_host(want).reshape(B, ow))}

    operands = {"a": (zeros(2 * l * N), "in"), "b": (zeros(b_words), "in"), "out": (zeros(ow), "out"), "key": ([key_host], "in"),
                "ws": ws_of(c.workspace_bytes(hg.OP_CKKS_LOGIC_GATE, depth, B))}
    call = lambda d, s: c.ckks_logic_gate(gate_id(hg, gate), d["a"], s["a"], d["b"], k, s["b"], d["key"], scale_one,  # noqa: E731
                                          d["out"], s["out"], depth, B, d["ws"])
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


@pytest.mark.parametrize("gate,kind", [("AND", "cipher"), ("XOR", "plain")])
def test_bfv_logic_gate(hg, torch, gate, kind):
    """bfv_logic_gate, method I, t = 65537: bfv_multiply + bfv_relinearize_inplace or bfv_multiply_plain, then the
    additions (chain_tail) of test_gpu_logic.py::test_bfv_logic_gate_equals_its_composition"""
    from test_gpu_logic import BFV_SETS, CIPHER, PLAIN, T, chain_tail, context, gate_id
    c, primes = context(hg, hg.BFV, *BFV_SETS["method_I"])
    Q = c.Q_size
    words = 2 * Q * N
    k = CIPHER if kind == "cipher" else PLAIN
    b_words = words if k == CIPHER else N
    key_host = synth_key(primes, c.switch_key_digits(), c.Q_prime_size, N, 5)
    key = hg.to_device(key_host)

    def case(seed):
        a = [synth_ct(primes, range(Q), 2, N, seed + i) for i in range(B)]
        if k == CIPHER:
            b = [synth_ct(primes, range(Q), 2, N, seed + 20 + i) for i in range(B)]
        else:
            b = [np.random.default_rng(seed + i).integers(0, T, N).astype(np.uint64) for i in range(B)]
        da, db = packed(hg, a), packed(hg, b)
        if k == CIPHER:
            prod = torch.empty(B * 3 * Q * N, dtype=torch.int64, device="cuda")
            c.bfv_multiply(da, words, db, words, prod, 3 * Q * N, B, c.workspace(hg.OP_BFV_MULTIPLY, 0, B))
            c.bfv_relinearize_inplace(prod, 3 * Q * N, key, B, c.workspace(hg.OP_BFV_RELIN, 0, B))
            p = prod.view(B, 3 * Q * N)[:, :words].contiguous().view(-1)
        else:
            p = torch.empty(B * words, dtype=torch.int64, device="cuda")
            w1 = c.workspace(hg.OP_BFV_MULTIPLY_PLAIN, 0, 1)
            for i in range(B):
                c._call("bfv_multiply_plain", da[i * words:].data_ptr(), db[i * N:].data_ptr(), p[i * words:].data_ptr(),
                        w1.data_ptr(), w1.numel() * 8)
        want = chain_tail(c, hg, torch, True, gate, da, db, k, p, Q, B, 0.0)
        torch.cuda.synchronize()
        return {"a": a, "b": b}, {"out": list(hg.to_host(want).reshape(B, words))}

    operands = {"a": (zeros(words), "in"), "b": (zeros(b_words), "in"), "out": (zeros(words), "out"), "key": ([key_host], "in"),
                "ws": ws_of(c.workspace_bytes(hg.OP_BFV_LOGIC_GATE, 0, B))}
    call = lambda d, s: c.bfv_logic_gate(gate_id(hg, gate), d["a"], s["a"], d["b"], k, s["b"], d["key"], d["out"], s["out"],  # noqa: E731
                                         B, d["ws"])
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ multiparty merges
def _share_ptrs(hg, views):
    import ctypes
    return (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])


def test_mpc_ckks_decrypt_merge(hg, oracle, torch):
    """mpc_ckks_decrypt_merge, three shares at depth 1: c0 plus the modular sum of the shares, limb by limb (the model of
    test_gpu_mpc.py::test_second_share_group_and_strides_that_differ)"""
    c, o, primes = ckks(hg, oracle, [50, 30, 30, 30], [50])
    depth, k = 1, 3
    l = c.Q_size - depth
    q = np.array(primes[:l], dtype=np.uint64).reshape(l, 1)

    def case(seed):
        g = np.random.default_rng(seed)
        res = lambda parts: np.stack([g.integers(0, primes[j], (parts, N), dtype=np.uint64) for j in range(l)], axis=1)  # noqa: E731
        cts = [res(2) for _ in range(B)]                      # [2][l][N]
        hs = [[res(1)[0] for _ in range(B)] for _ in range(k)]  # per share, per item [l][N]
        want = []
        for b in range(B):
            acc = cts[b][0]
            for h in hs:
                acc = (acc + h[b]) % q
            want.append(acc.reshape(-1))
        inputs = {"ct": [x.reshape(-1) for x in cts]}
        inputs.update({"h%d" % i: [np.concatenate([x.reshape(-1) for x in h])] for i, h in enumerate(hs)})
        return inputs, {"plain": [np.concatenate(want)]}

    # the shares and the result are contiguous batches (the ABI gives them no stride): one item each
    operands = {"ct": (zeros(2 * l * N), "in"), "plain": (zeros(B * l * N, 1), "out")}
    operands.update({"h%d" % i: (zeros(B * l * N, 1), "in") for i in range(k)})
    call = lambda d, s: c._call("mpc_ckks_decrypt_merge", d["ct"].data_ptr(), s["ct"],  # noqa: E731
                                _share_ptrs(hg, [d["h%d" % i] for i in range(k)]), k, depth, d["plain"].data_ptr(), B)
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_mpc_bfv_decrypt_merge(hg, oracle, torch):
    """mpc_bfv_decrypt_merge on the decryption shares of two parties, made before the capture: the merge opens the two
    messages that were encrypted under the collective public key (test_gpu_mpc.py::test_bfv_collective_keys_and_decryption)"""
    from test_gpu_mpc import Parties
    c, o, primes, t = bfv(hg, oracle)
    Q, k = c.Q_size, 2
    words = 2 * Q * N
    p = Parties(hg, c, k)
    pk = p.public_key()

    def case(seed):
        g = np.random.default_rng(seed)
        msgs = g.integers(0, t, (B, N)).astype(np.uint64)
        enc = hg.Rng(1000 + seed)
        cts = [hg.to_host(c.bfv_encrypt(enc, pk, hg.to_device(m))) for m in msgs]
        dct = packed(hg, cts)
        hs = [hg.to_host(c.mpc_bfv_decrypt_share(p.rng[i], dct, words, p.sk[i], B)) for i in range(k)]
        inputs = {"ct": cts}
        inputs.update({"h%d" % i: [h] for i, h in enumerate(hs)})
        return inputs, {"plain": [msgs.reshape(-1)]}

    nbytes = c.workspace_bytes(hg.OP_MPC_BFV_DECRYPT_MERGE, 0, B)
    operands = {"ct": (zeros(words), "in"), "plain": (zeros(B * N, 1), "out"), "ws": ws_of(nbytes)}
    operands.update({"h%d" % i: (zeros(B * Q * N, 1), "in") for i in range(k)})
    call = lambda d, s: c._call("mpc_bfv_decrypt_merge", d["ct"].data_ptr(), s["ct"],  # noqa: E731
                                _share_ptrs(hg, [d["h%d" % i] for i in range(k)]), k, d["plain"].data_ptr(), B,
                                d["ws"].data_ptr(), d["ws"].numel() * 8)
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_mpc_refresh_merge(hg, oracle, torch, scheme):
    """mpc_ckks_refresh_merge (depth 1) and mpc_bfv_refresh_merge on two arbitrary share arrays: the replay against the
    eager call, which test_gpu_mpc_refresh.py::test_ckks_coordinator_is_exact / test_bfv_coordinator_is_exact pin to
    Python integers on arbitrary shares.  The merge derives the public `a` from the common generator's counter as it
    stands at the call: every call here gets a generator fresh from the common seed, as the parties' shares would."""
    CRS, k = 4242, 2
    if scheme == "ckks":
        c, o, primes = ckks(hg, oracle, [50, 30, 30, 30], [50])
        depth = 1
    else:
        c, o, primes, _ = bfv(hg, oracle)
        depth = 0
    Q = c.Q_size
    l = Q - depth
    in_words, out_words = 2 * l * N, 2 * Q * N
    share_words = (l + Q) * N if scheme == "ckks" else 2 * Q * N
    rows = list(range(l)) + list(range(Q)) if scheme == "ckks" else list(range(Q)) * 2
    nbytes = c.workspace_bytes(hg.OP_MPC_REFRESH_MERGE, depth, B)

    def merge(ct, cs, shares, out, so, ws):
        crs = hg.Rng(CRS)  # alive until the call has returned
        head = (crs._h, ct.data_ptr(), cs, _share_ptrs(hg, shares), k)
        tail = (out.data_ptr(), so, B, ws.data_ptr(), ws.numel() * 8)
        if scheme == "ckks":
            c._call("mpc_ckks_refresh_merge", *head, depth, *tail)
        else:
            c._call("mpc_bfv_refresh_merge", *head, *tail)

    def case(seed):
        g = np.random.default_rng(seed)
        cts = [np.concatenate([g.integers(0, primes[j], N, dtype=np.uint64) for j in list(range(l)) * 2]) for _ in range(B)]
        hs = [np.concatenate([g.integers(0, primes[j], N, dtype=np.uint64) for _ in range(B) for j in rows]) for _ in range(k)]
        out = torch.zeros(B * out_words, dtype=torch.int64, device="cuda")
        merge(packed(hg, cts), in_words, [hg.to_device(h) for h in hs], out, out_words,
              torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        inputs = {"ct": cts}
        inputs.update({"h%d" % i: [h] for i, h in enumerate(hs)})
        return inputs, {"out": list(hg.to_host(out).reshape(B, out_words))}

    operands = {"ct": (zeros(in_words), "in"), "out": (zeros(out_words), "out"), "ws": ws_of(nbytes)}
    operands.update({"h%d" % i: (zeros(B * share_words, 1), "in") for i in range(k)})
    call = lambda d, s: merge(d["ct"], s["ct"], [d["h%d" % i] for i in range(k)], d["out"], s["out"], d["ws"])  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ encoders
@pytest.mark.parametrize("n,log_q", [(4096, [50, 40, 40]), (16384, [60, 50, 50, 50, 50])], ids=["n4096", "n16384_chunked_fft"])
def test_ckks_encode_and_decode(hg, oracle, torch, n, log_q):
    """ckks_encode -> ckks_decode of the encoded plaintext; N = 2^14 takes the chunked FFT with 128 KiB of dynamic LDS (its
    function attribute is set by a static on the first call).  The oracle's residues and doubles bit for bit
    (tests/test_gpu_encode.py::test_encode_decode_match_oracle)"""
    c, o, primes = ckks(hg, oracle, log_q, [60], n)
    Q, slots, scale = len(log_q), n // 2, 2.0 ** 40
    enc_bytes, dec_bytes = c.workspace_bytes(hg.OP_CKKS_ENCODE, 0, 1), c.workspace_bytes(hg.OP_CKKS_DECODE, 0, 1)

    def case(seed):
        msg = np.random.default_rng(seed).uniform(-100, 100, slots)
        plain = o.ckks_encode(msg, scale)
        return {"msg": [msg]}, {"plain": [plain], "back": [o.ckks_decode(plain, scale, 0)]}

    operands = {"msg": (zeros(slots, 1, np.float64), "in"), "plain": (zeros(Q * n, 1), "out"),
                "back": (zeros(slots, 1, np.float64), "out"), "ws_enc": ws_of(enc_bytes), "ws_dec": ws_of(dec_bytes)}

    def call(d, s):
        c._call("ckks_encode", d["msg"].data_ptr(), slots, scale, d["plain"].data_ptr(), d["ws_enc"].data_ptr(), enc_bytes)
        c._call("ckks_decode", d["plain"].data_ptr(), 0, scale, d["back"].data_ptr(), d["ws_dec"].data_ptr(), dec_bytes)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_bfv_encode_and_decode(hg, oracle, torch):
    """bfv_encode -> bfv_decode of the encoded plaintext, t = 1032193: the oracle's words"""
    c, o, primes, t = bfv(hg, oracle)
    dec_bytes = c.workspace_bytes(hg.OP_BFV_DECODE, 0, 1)

    def case(seed):
        msg = np.random.default_rng(seed).integers(0, t, N).astype(np.int64)
        msg[:3] = [0, t - 1, t // 2]
        plain = o.bfv_encode(msg)
        return {"msg": [msg]}, {"plain": [plain], "back": [o.bfv_decode(plain)]}

    operands = {"msg": (zeros(N, 1, np.int64), "in"), "plain": (zeros(N, 1), "out"), "back": (zeros(N, 1), "out"),
                "ws": ws_of(dec_bytes)}

    def call(d, s):
        c._call("bfv_encode", d["msg"].data_ptr(), N, d["plain"].data_ptr())
        c._call("bfv_decode", d["plain"].data_ptr(), d["back"].data_ptr(), d["ws"].data_ptr(), dec_bytes)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ the kernel seam
@pytest.mark.parametrize("single", [1, 0], ids=["single_pass", "two_pass"])
def test_ntt_in_place(hg, oracle, torch, single):
    """hegpu_ntt forward and inverse, both in place, on {60, 45 | 60} (an integer and an FP64 modulus), seven polynomials
    that wrap around the modulus list: the oracle's transform, and its input back"""
    from helpers import backend_switches
    tag = ("ntt", single)
    if tag not in _made:
        with backend_switches(HEGPU_SINGLE_PASS=single):
            c = hg.Context.from_bit_sizes(hg.CKKS, N, [60, 45], [60], sec=hg.SEC_NONE)
        primes = [int(x) for x in c.table("modulus")]
        c.upload()
        _made[tag] = (c, oracle.OracleContext(oracle.CKKS, c.n_power, primes, 2, 1), primes)
    c, o, primes = _made[tag]
    Qp, batch = 3, 7

    def case(seed):
        x = np.concatenate([oracle.fill_poly(seed + i, i % Qp, N, primes[i % Qp]) for i in range(batch)])
        x[:4] = [0, primes[0] - 1, 1, primes[0] // 2]
        y = o.ntt(x.copy(), batch, Qp)
        return {"fwd": [x], "inv": [y]}, {"fwd": [y], "inv": [x]}

    operands = {"fwd": (zeros(batch * N, 1), "inout"), "inv": (zeros(batch * N, 1), "inout")}

    def call(d, s):
        c.ntt(d["fwd"], d["fwd"], False, batch, Qp)
        c.ntt(d["inv"], d["inv"], True, batch, Qp)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_addition_cross_and_cipherplain_multiplication(hg, oracle, torch):
    """the kernel entries addition (add), cross_multiplication and cipherplain_multiplication at three limbs of
    {60, 40, 45, 40 | 60}: the oracle's kernels, the plain product in Python integers
    (tests/test_gpu_reference_kernels.py::test_cipherplain_multiplication)"""
    from test_gpu_kernels import _limbs
    c, o, primes = ckks(hg, oracle, [60, 40, 45, 40], [60])
    L = 3
    per = 2 * L * N
    mods = o.mods(primes)

    def case(seed):
        a = [synth_ct(primes, range(L), 2, N, seed + 10 * b) for b in range(B)]
        b_ = [synth_ct(primes, range(L), 2, N, seed + 10 * b + 5) for b in range(B)]
        plain = _limbs(oracle, primes, range(L), N, seed + 40)
        fa, fb = np.concatenate(a), np.concatenate(b_)
        total = np.zeros_like(fa)
        for i in range(B):
            o.L.o_addition(fa[i * per:].ctypes.data, fb[i * per:].ctypes.data, total[i * per:].ctypes.data, mods, 12, L, 2)
        cross = []
        for i in range(B):
            w = np.zeros(3 * L * N, dtype=np.uint64)
            o.L.o_cross_multiplication(a[i].ctypes.data, b_[i].ctypes.data, w.ctypes.data, mods, 12, L)
            cross.append(w)
        cp = np.zeros(per, dtype=np.uint64)
        for z in range(2):
            for j in range(L):
                at = (z * L + j) * N
                cp[at:at + N] = np.array((a[0][at:at + N].astype(object) * plain[j * N:(j + 1) * N].astype(object)) % primes[j],
                                         dtype=np.uint64)
        return ({"a": a, "b": b_, "fa": [fa], "fb": [fb], "plain": [plain]}, {"sum": [total], "cross": cross, "cp": [cp]})

    # hegpu_addition takes no stride: its batch is contiguous, one item here
    operands = {"a": (zeros(per), "in"), "b": (zeros(per), "in"), "fa": (zeros(B * per, 1), "in"), "fb": (zeros(B * per, 1), "in"),
                "plain": (zeros(L * N, 1), "in"), "sum": (zeros(B * per, 1), "out"), "cross": (zeros(3 * L * N), "out"),
                "cp": (zeros(per, 1), "out")}

    def call(d, s):
        c.addition(d["fa"], d["fb"], d["sum"], L, 2, B, 0)
        c.cross_multiplication(d["a"], s["a"], d["b"], s["b"], d["cross"], s["cross"], L, B)
        c._call("cipherplain_multiplication", d["a"].data_ptr(), d["plain"].data_ptr(), d["cp"].data_ptr(), L)

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ TFHE
def _tfhe(hg, oracle):
    """a context, the oracle, a torus32 boot key prepared before any capture, and key-switch keys"""
    if "tfhe" not in _made:
        t, o = hg.TfheContext(), oracle.OracleTfhe()
        g = np.random.default_rng(11)
        polys = t.int("bootkey_elems") // 1024
        coeff = g.integers(-2 ** 31, 2 ** 31, (polys, 1024), dtype=np.int64).astype(np.int32)
        bk = np.concatenate([o.to_ntt(coeff[i]) for i in range(polys)])
        prepared = t.prepare_bootkey(hg.to_device(bk))
        assert t.prepared_is_fp64(prepared)
        ks_a = g.integers(-2 ** 31, 2 ** 31, t.int("kskey_a_elems"), dtype=np.int64).astype(np.int32)
        ks_b = g.integers(-2 ** 31, 2 ** 31, t.int("kskey_b_elems"), dtype=np.int64).astype(np.int32)
        _made["tfhe"] = (t, o, bk, prepared, ks_a, ks_b)
    return _made["tfhe"]


def _torus(g, count):
    return g.integers(-2 ** 31, 2 ** 31, count, dtype=np.int64).astype(np.int32)


def _wrap(x):
    return (x.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def test_tfhe_gate_and_mux(hg, oracle, torch):
    """tfhe_gate (NAND) and tfhe_mux on three gates, torus32 key: the oracle's gate; the MUX from the oracle's parts as
    hegpu.h states it -- AND(c, in1) and AND(NOT c, in2) bootstrapped, the OR pre-computation of the two extracted samples
    (their sum plus 1/8), the key switch"""
    t, o, bk, prepared, ks_a, ks_b = _tfhe(hg, oracle)
    S, n, kN = 3, 512, 1024

    def case(seed):
        g = np.random.default_rng(seed)
        a1, a2, ca = _torus(g, S * n), _torus(g, S * n), _torus(g, S * n)
        b1, b2, cb = _torus(g, S), _torus(g, S), _torus(g, S)
        nand_a, nand_b = o.gate(hg.GATE_NAND, a1, b1, a2, b2, bk, ks_a, ks_b)
        e1a, e1b = o.bootstrapping(*o.gate_pre(hg.GATE_AND, ca, cb, a1, b1), bk)
        e2a, e2b = o.bootstrapping(*o.gate_pre(hg.GATE_AND_FIRST_NOT, ca, cb, a2, b2), bk)
        ea = _wrap(e1a.astype(np.int64) + e2a)
        eb = _wrap(e1b.astype(np.int64) + e2b + o.mu)
        mux_a, mux_b = o.key_switching(ea, eb, ks_a, ks_b)
        return ({"a1": [a1], "b1": [b1], "a2": [a2], "b2": [b2], "ca": [ca], "cb": [cb]},
                {"nand_a": [nand_a], "nand_b": [nand_b], "mux_a": [mux_a], "mux_b": [mux_b]})

    i32 = lambda count, kind: (zeros(count, 1, np.int32), kind)  # noqa: E731
    operands = {"a1": i32(S * n, "in"), "b1": i32(S, "in"), "a2": i32(S * n, "in"), "b2": i32(S, "in"), "ca": i32(S * n, "in"),
                "cb": i32(S, "in"), "nand_a": i32(S * n, "out"), "nand_b": i32(S, "out"), "mux_a": i32(S * n, "out"),
                "mux_b": i32(S, "out"), "ks_a": ([ks_a], "in"), "ks_b": ([ks_b], "in"),
                "ws_gate": i32((n + kN + 2) * S, "ws"), "ws_mux": i32((n + 1 + 2 * (kN + 1)) * S, "ws")}

    def call(d, s):
        t.gate(hg.GATE_NAND, d["a1"], d["b1"], d["a2"], d["b2"], d["nand_a"], d["nand_b"], prepared, d["ks_a"], d["ks_b"], S,
               d["ws_gate"])
        t.mux(d["a1"], d["b1"], d["a2"], d["b2"], d["ca"], d["cb"], d["mux_a"], d["mux_b"], prepared, d["ks_a"], d["ks_b"], S,
              d["ws_mux"])

    parity(torch, operands, call, [case(seed) for seed in SEEDS])


def test_tfhe_key_switching_batched(hg, oracle, torch):
    """tfhe_key_switching at 48 gates: 16 gates per workgroup, the coefficient loop cut into pieces that add their partial
    sums atomically onto outputs cleared first on the caller's stream -- over poisoned outputs a clear that went
    elsewhere shows.  (This test found the clear, then a hipMemsetAsync, replayed with a stale fill value from the second
    replay on: a captured memset node of 16 bytes or more does that on its own; the entry now clears with a kernel.)
    Every gate against the eager call on the null stream, of which four gates are the oracle's
    (tests/test_gpu_tfhe.py::test_key_switching_split_launches; the oracle takes seconds per gate)"""
    t, o, bk, prepared, ks_a, ks_b = _tfhe(hg, oracle)
    S, n, kN = 48, 512, 1024
    dks_a, dks_b = torch.from_numpy(ks_a).cuda(), torch.from_numpy(ks_b).cuda()

    def case(seed):
        g = np.random.default_rng(seed)
        ea, eb = _torus(g, S * kN), _torus(g, S)
        ka = torch.full((S * n,), 7, dtype=torch.int32, device="cuda")
        kb = torch.full((S,), 7, dtype=torch.int32, device="cuda")
        t.key_switching(torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda(), ka, kb, dks_a, dks_b, S)
        torch.cuda.synchronize()
        got_a, got_b = ka.cpu().numpy(), kb.cpu().numpy()
        for gate in (0, 1, 17, S - 1):
            want_a, want_b = o.key_switching(ea[gate * kN:(gate + 1) * kN], eb[gate:gate + 1], ks_a, ks_b)
            assert np.array_equal(got_a[gate * n:(gate + 1) * n], want_a) and got_b[gate] == want_b[0], gate
        return {"ea": [ea], "eb": [eb]}, {"ka": [got_a], "kb": [got_b]}

    i32 = lambda count, kind: (zeros(count, 1, np.int32), kind)  # noqa: E731
    operands = {"ea": i32(S * kN, "in"), "eb": i32(S, "in"), "ka": i32(S * n, "out"), "kb": i32(S, "out"),
                "ks_a": ([ks_a], "in"), "ks_b": ([ks_b], "in")}
    call = lambda d, s: t.key_switching(d["ea"], d["eb"], d["ka"], d["kb"], d["ks_a"], d["ks_b"], S)  # noqa: E731
    parity(torch, operands, call, [case(seed) for seed in SEEDS])


# ------------------------------------------------------------------ entries that must not be captured
def test_drawing_and_synchronising_entries_refuse_a_capturing_stream(hg, oracle, torch):
    """Inside a capture ckks_encrypt, generate_public_key, mpc_public_key_share, tfhe_encrypt, generate_secret_key and
    tfhe_prepare_bootkey raise HEError(E_LOGIC) and say why.  The capture survives: a ckks_multiply recorded behind the
    refusals replays to the oracle's product on two inputs.  The generators did not move: after the refused call each
    gives what an equally seeded generator gives that was never refused."""
    c, o, primes = ckks(hg, oracle, [40, 30, 30], [40])
    Q = c.Q_size
    words = 2 * Q * N
    setup = hg.Rng(5)
    sk = c.generate_secret_key(setup)
    pk = c.generate_public_key(setup, sk)
    plain = hg.to_device(synth_ct(primes, range(Q), 1, N, 9))
    t = hg.TfheContext()
    lwe, _ = t.generate_secret_key(setup)
    messages = torch.from_numpy(np.array([1 << 29, -(1 << 29), 1 << 29], dtype=np.int32)).cuda()
    boot_key = hg.to_device(np.random.default_rng(2).integers(0, t.prime, t.int("bootkey_elems"), dtype=np.uint64))
    t.prepare_bootkey(boot_key)  # the context's tables are placed outside the capture
    cat = lambda x: torch.cat([v.reshape(-1).to(torch.int64) for v in x]) if isinstance(x, tuple) else x  # noqa: E731
    draws = {
        "ckks_encrypt": lambda r: c.ckks_encrypt(r, pk, plain),
        "generate_public_key": lambda r: c.generate_public_key(r, sk),
        "mpc_public_key_share": lambda r: c.mpc_public_key_share(hg.Rng(4242), r, sk),
        "tfhe_encrypt": lambda r: cat(t.encrypt(r, lwe, messages)),
        "generate_secret_key": lambda r: c.generate_secret_key(r),
    }
    refused = {name: hg.Rng(700 + i) for i, name in enumerate(draws)}
    control = {name: hg.Rng(700 + i) for i, name in enumerate(draws)}
    d1, d2 = torch.zeros(words, dtype=torch.int64, device="cuda"), torch.zeros(words, dtype=torch.int64, device="cuda")
    out = torch.zeros(3 * Q * N, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # warm-up of everything the capture touches
        c.ckks_multiply(d1, words, d2, words, out, 3 * Q * N, 0, 1)
        for name, fn in draws.items():
            fn(hg.Rng(1))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for name, fn in draws.items():
            with pytest.raises(hg.HEError) as e:
                fn(refused[name])
            assert e.value.code == hg.E_LOGIC, (name, e.value)
            why = "synchronises" if name == "generate_secret_key" else "draws randomness"
            assert why in str(e.value) and name in str(e.value), (name, e.value)
        with pytest.raises(hg.HEError) as e:
            t.prepare_bootkey(boot_key)
        assert e.value.code == hg.E_LOGIC and "synchronises" in str(e.value), e.value
        with pytest.raises(hg.HEError) as e:
            t.status()
        assert e.value.code == hg.E_LOGIC and "synchronises" in str(e.value), e.value
        c.ckks_multiply(d1, words, d2, words, out, 3 * Q * N, 0, 1)
    for seed in SEEDS:
        ct1, ct2 = synth_ct(primes, range(Q), 2, N, seed), synth_ct(primes, range(Q), 2, N, seed + 1)
        d1.copy_(hg.to_device(ct1))
        d2.copy_(hg.to_device(ct2))
        out.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(hg.to_host(out), o.ckks_multiply(ct1, ct2, 0)), "a multiply captured behind the refusals"
    for name, fn in draws.items():
        got, want = fn(refused[name]), fn(control[name])
        torch.cuda.synchronize()
        assert torch.equal(got, want), name + ": the refused call moved the generator"
