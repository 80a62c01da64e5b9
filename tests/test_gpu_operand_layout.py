"""Every entry on operands that are only 8-byte aligned and on odd item strides (helpers.laid_out, helpers.LAYOUTS).

include/hegpu.h asks for no more than the alignment of the element type and an item stride not smaller than the item.
The streaming kernels of rns.hip move pairs of coefficients with 16-byte accesses wherever the operand lies; the fused
row pass of the key switch (ntt.hip ks_row_mac_launch, pair_ok) chooses between its wide and its natural kernels by the
low bits of the pointers and strides of each launch.  Either way the residues must be the CPU oracle's bit for bit, the
inputs must stay as they were and nothing outside the operands may be written: every operand sits between sentinel
words, the one directly in front of it included (a kernel that rounded an address down to 16 bytes would overwrite it or
return shifted data).

Shapes: A = CKKS N = 2^12 {60, 40, 45, 40 | 60} (FP64 and integer moduli, the integer special prime takes the mod-down
tail), B = CKKS N = 2^12 {50, 36 x 4 | 50, 50} (method II, three digits), C = BFV N = 2^12 default chain, D = A's chain
at N = 2^15 (two-pass transforms, eight tiles per row kernel).  Contexts and references are made once per module.

The launches of the fused row pass per call, and the operands each of them moves in pairs (ops.cpp):
  A, relinearize / apply_galois: the special-prime slot first -- key, the accumulator in the workspace, the identity limb
     of the input -- then the Q slots with the mod-down tail -- key, identity limb and added part of the input, output;
  B and C: one launch -- key and the accumulator in the workspace (no identity limb, the mod-down is a later launch);
  hoisted rotations of more than one element: none (shared digits, element-wise inner products).
A launch is natural exactly when one of its operands is 8 bytes off or has an odd stride, else wide; so a workspace 8
bytes off turns the launches that keep their accumulator there natural and leaves the tail launch, which reads the
workspace 8 bytes per lane, wide."""
import numpy as np
import pytest

from helpers import LAYOUTS, extreme_limbs, items_of, laid_out, synth_ct, synth_key
from test_gpu_kernels import _limbs, _rescale_location
from test_gpu_mod_raise import planted, want_raise

pytestmark = pytest.mark.gpu

N = 4096
B = 3  # items per launch: in the odd layouts items 0 and 2 are aligned, item 1 is 8 bytes off (or the other way round)
SHAPES = {
    "A": ([60, 40, 45, 40], [60]),
    "B": ([50, 36, 36, 36, 36], [50, 50]),
}
SETTINGS = {
    "default": dict(fused_row_mac=-1, digit_split=-1, col_multi=-1),
    "forced_col0": dict(fused_row_mac=1, digit_split=0, col_multi=0),
    "forced_col1": dict(fused_row_mac=1, digit_split=0, col_multi=1),
    "split2": dict(fused_row_mac=-1, digit_split=2, col_multi=-1),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_shapes = {}


def shape(hg, oracle, name):
    """(context, oracle context, primes) of shape A, B, C or D"""
    if name not in _shapes:
        if name == "C":
            c = hg.Context.from_default(hg.BFV, N, 1, 1032193)
            primes = [int(x) for x in c.table("modulus")]
            o = oracle.OracleContext(oracle.BFV, c.n_power, primes, c.Q_size, c.P_size, 1032193)
        else:
            log_q, log_p = SHAPES["A" if name == "D" else name]
            c = hg.Context.from_bit_sizes(hg.CKKS, 1 << 15 if name == "D" else N, log_q, log_p, sec=hg.SEC_NONE)
            primes = [int(x) for x in c.table("modulus")]
            o = oracle.OracleContext(oracle.CKKS, c.n_power, primes, len(log_q), len(log_p))
        c.upload()
        _shapes[name] = (c, o, primes)
    return _shapes[name]


def _outs(words, count=B):
    return [np.full(words, 7, dtype=np.uint64) for _ in range(count)]


def _ws(c, op, depth, batch):
    """a workspace as an operand: exactly workspace_bytes bytes between the sentinels"""
    return ([np.zeros(max(c.workspace_bytes(op, depth, batch) // 8, 1), dtype=np.uint64)], "ws")


def _run(torch, operands, place, call):
    """operands: name -> (items, kind), kind "in" (must stay unchanged), "out" / "inout" (returned), "ws"; place(name) ->
    (lead, pad).  call(d, s) gets the device views and the item strides.  Returns name -> [items][words] of the outputs."""
    dev = {name: laid_out(items, *place(name)) for name, (items, _) in operands.items()}
    call({k: v[0] for k, v in dev.items()}, {k: v[1] for k, v in dev.items()})
    torch.cuda.synchronize()
    got = {}
    for name, (items, kind) in operands.items():
        view, stride, intact = dev[name]
        assert intact(), "written outside the operand " + name
        if kind == "ws":
            continue
        now = items_of(view, stride, len(items[0]), len(items))
        if kind == "in":
            assert np.array_equal(now, np.stack(items)), "input changed: " + name
        else:
            got[name] = now
    return got


def _compare(got, want, tag):
    """want: name -> per item the expected leading words"""
    for name, rows in want.items():
        for b, w in enumerate(rows):
            assert np.array_equal(got[name][b][:len(w)], w), (tag, name, b)


# ------------------------------------------------------------------ (a) streaming kernels
# Each row builds (operands, call, want) once; the oracle calls are those of tests/test_gpu_kernels.py (tests/
# test_gpu_parity.py for the additions, tests/test_gpu_mod_raise.py for the raise).
def row_addition(hg, oracle, op):
    c, o, primes = shape(hg, oracle, "C")
    Q, per = c.Q_size, 2 * c.Q_size * N
    a = np.concatenate([synth_ct(primes, range(Q), 2, N, 1 + b) for b in range(B)])
    b_ = np.concatenate([synth_ct(primes, range(Q), 2, N, 40 + b) for b in range(B)])
    a[5] = 0  # negation of zero
    want = np.zeros_like(a)
    for i in range(B):
        if op == 2:
            o.L.o_negation(a[i * per:].ctypes.data, want[i * per:].ctypes.data, o.qp_mods, 12, Q, 2)
        else:
            fn = (o.L.o_addition, o.L.o_substraction)[op]
            fn(a[i * per:].ctypes.data, b_[i * per:].ctypes.data, want[i * per:].ctypes.data, o.qp_mods, 12, Q, 2)
    ops = {"a": ([a], "in"), "b": ([b_], "in"), "out": (_outs(len(a), 1), "out")}
    call = lambda d, s: c.addition(d["a"], None if op == 2 else d["b"], d["out"], Q, 2, B, op)
    return ops, call, {"out": [want]}


def row_cross_multiplication(hg, oracle, merged):
    c, o, primes = shape(hg, oracle, "C")
    mods_list = [int(v) for v in c.table("q_Bsk_merge_modulus")] if merged else primes
    L = len(mods_list)
    a = [_limbs(oracle, mods_list, list(range(L)) * 2, N, 11 + b) for b in range(B)]
    b_ = [_limbs(oracle, mods_list, list(range(L)) * 2, N, 31 + b) for b in range(B)]
    mods = o.mods(mods_list)
    want = []
    for b in range(B):
        w = np.zeros(3 * L * N, dtype=np.uint64)
        o.L.o_cross_multiplication(a[b].ctypes.data, b_[b].ctypes.data, w.ctypes.data, mods, 12, L)
        want.append(w)
    ops = {"in1": (a, "in"), "in2": (b_, "in"), "out": (_outs(3 * L * N), "out")}
    ts = hg.TABLES_Q_BSK if merged else hg.TABLES_QP
    call = lambda d, s: c.cross_multiplication(d["in1"], s["in1"], d["in2"], s["in2"], d["out"], s["out"], L, B, table_set=ts)
    return ops, call, {"out": want}


def row_cipher_broadcast(hg, oracle, leveled):
    if not leveled:
        c, o, primes = shape(hg, oracle, "C")
        Q, Qp = c.Q_size, c.Q_prime_size
        src = [_limbs(oracle, primes, range(Q), N, 5 + b) for b in range(B)]
        want = []
        for b in range(B):
            w = np.zeros(Q * Qp * N, dtype=np.uint64)
            o.L.o_cipher_broadcast(src[b].ctypes.data, w.ctypes.data, o.qp_mods, 12, Q, Qp)
            want.append(w)
        ops = {"src": (src, "in"), "out": (_outs(Q * Qp * N), "out")}
        call = lambda d, s: c.cipher_broadcast(d["src"], s["src"], d["out"], s["out"], Q, Qp, Qp, 0, B)
        return ops, call, {"out": want}
    c, o, primes = shape(hg, oracle, "A")
    depth = 1
    Qp = c.Q_prime_size
    l, rc = c.Q_size - depth, Qp - depth
    src = [_limbs(oracle, primes, range(l), N, 9 + b) for b in range(B)]
    want = []
    for b in range(B):
        w = np.zeros(l * rc * N, dtype=np.uint64)
        o.L.o_cipher_broadcast_leveled(src[b].ctypes.data, w.ctypes.data, o.qp_mods, Qp, rc, 12, l)
        want.append(w)
    ops = {"src": (src, "in"), "out": (_outs(l * rc * N), "out")}
    call = lambda d, s: c.cipher_broadcast(d["src"], s["src"], d["out"], s["out"], l, rc, l, depth, B)
    return ops, call, {"out": want}


def row_keyswitch_mac(hg, oracle, leveled):
    if not leveled:
        c, o, primes = shape(hg, oracle, "C")
        Q, Qp = c.Q_size, c.Q_prime_size
        key = synth_key(primes, Q, Qp, N, 3)
        dig = [np.concatenate([_limbs(oracle, primes, range(Qp), N, 70 + 7 * b + d) for d in range(Q)]) for b in range(B)]
        want = []
        for b in range(B):
            w = np.zeros(2 * Qp * N, dtype=np.uint64)
            o.L.o_keyswitch_mac(dig[b].ctypes.data, key.ctypes.data, w.ctypes.data, o.qp_mods, 12, Qp, Q)
            want.append(w)
        ops = {"dig": (dig, "in"), "key": ([key], "in"), "acc": (_outs(2 * Qp * N), "out")}
        call = lambda d, s: c.keyswitch_multiply_accumulate(d["dig"], s["dig"], d["key"], d["acc"], s["acc"], Q, Qp, Qp, Qp, 0, B)
        return ops, call, {"acc": want}
    c, o, primes = shape(hg, oracle, "A")
    depth = 1
    Q, Qp = c.Q_size, c.Q_prime_size
    l, rc = Q - depth, Qp - depth
    key = synth_key(primes, Q, Qp, N, 3)
    limb_ids = list(range(l)) + [Q]  # rows 0..l-1 use q_y, row l the special prime
    dig = [np.concatenate([_limbs(oracle, primes, limb_ids, N, 40 + 7 * b + d) for d in range(l)]) for b in range(B)]
    want = []
    for b in range(B):
        w = np.zeros(2 * rc * N, dtype=np.uint64)
        o.L.o_keyswitch_mac_leveled(dig[b].ctypes.data, key.ctypes.data, w.ctypes.data, o.qp_mods, Qp, l, 12)
        want.append(w)
    ops = {"dig": (dig, "in"), "key": ([key], "in"), "acc": (_outs(2 * rc * N), "out")}
    call = lambda d, s: c.keyswitch_multiply_accumulate(d["dig"], s["dig"], d["key"], d["acc"], s["acc"], l, rc, Qp, l, depth, B)
    return ops, call, {"acc": want}


def row_base_conversion(hg, oracle, depth):
    c, o, primes = shape(hg, oracle, "B")
    Q, P = c.Q_size, c.P_size
    l, rc = Q - depth, Q + P - depth
    dg = -(-l // P)
    src = [_limbs(oracle, primes, range(l), N, 21 + b) for b in range(B)]
    for s_ in src:
        s_[:3] = [0, primes[0] - 1, primes[0] // 2]
    want = []
    for b in range(B):
        w = np.zeros(dg * rc * N, dtype=np.uint64)
        o.L.o_base_conversion_DtoQtilde(o.h, src[b].ctypes.data, w.ctypes.data, depth)
        want.append(w)
    ops = {"src": (src, "in"), "out": (_outs(dg * rc * N), "out")}
    call = lambda d, s: c.base_conversion_DtoQtilde(d["src"], s["src"], d["out"], s["out"], depth, B)
    return ops, call, {"out": want}


def row_divide_round_lastq(hg, oracle, switchkey):
    c, o, primes = shape(hg, oracle, "C")
    Q, Qp = c.Q_size, c.Q_prime_size
    src = [_limbs(oracle, primes, list(range(Qp)) * 2, N, 3 + b) for b in range(B)]
    for s_ in src:
        s_[:4] = [0, primes[0] - 1, 1, primes[0] // 2]
        s_[Q * N:Q * N + 3] = [0, primes[Q] - 1, primes[Q] // 2]  # the P limb at its corners
    cts = [synth_ct(primes, range(Q), 2, N, 50 + b) for b in range(B)]
    half, half_mod, inv = o.table("half"), o.table("half_mod"), o.table("last_q_modinv")
    want = []
    for b in range(B):
        w = np.zeros(2 * Q * N, dtype=np.uint64)
        o.L.o_divide_round_lastq(src[b].ctypes.data, cts[b].ctypes.data, w.ctypes.data, o.qp_mods, half.ctypes.data,
                                 half_mod.ctypes.data, inv.ctypes.data, 12, Q, switchkey)
        want.append(w)
    ops = {"src": (src, "in"), "ct": (cts, "in"), "out": (_outs(2 * Q * N), "out")}
    call = lambda d, s: c.divide_round_lastq(d["src"], s["src"], d["ct"], s["ct"], d["out"], s["out"], switchkey, B)
    return ops, call, {"out": want}


def row_permute(hg, oracle, which, depth):
    c, o, primes = shape(hg, oracle, which)
    g = 3 if which == "C" else hg.steps_to_galois_elt(-2, N, 5)
    Q, Qp, P = c.Q_size, c.Q_prime_size, c.P_size
    l, rc = Q - depth, Qp - depth
    limb_ids = list(range(l)) + list(range(Q, Qp))
    src = [_limbs(oracle, primes, limb_ids * 2, N, 13 + b) for b in range(B)]
    for s_ in src:
        s_[0] = 0  # q - 0 = q is stored un-reduced by the reference's negation
    in2 = [_limbs(oracle, primes, range(l), N, 60 + b) for b in range(B)]
    half, half_mod, inv = o.table("half"), o.table("half_mod"), o.table("last_q_modinv")
    want = []
    for b in range(B):
        w = np.zeros(2 * l * N, dtype=np.uint64)
        o.L.o_divide_round_lastq_permute(src[b].ctypes.data, in2[b].ctypes.data, w.ctypes.data, o.qp_mods,
                                         half.ctypes.data, half_mod.ctypes.data, inv.ctypes.data, g, 12, rc, l, Qp, Q, P)
        want.append(w)
    ops = {"src": (src, "in"), "in2": (in2, "in"), "out": (_outs(2 * l * N), "out")}
    call = lambda d, s: c.divide_round_lastq_permute(d["src"], s["src"], d["in2"], s["in2"], d["out"], s["out"], g, depth, B)
    return ops, call, {"out": want}


def _moddown_inputs(oracle, c, primes, depth):
    Q = c.Q_size
    l = Q - depth
    ids = list(range(l)) + [Q]
    src = [_limbs(oracle, primes, ids * 2, N, 5 + b) for b in range(B)]
    for s_ in src:
        s_[l * N:l * N + 3] = [0, primes[Q] - 1, primes[Q] // 2]
    ct_in = [synth_ct(primes, range(l), 2, N, 90 + b) for b in range(B)]
    for s_ in ct_in:
        s_[(l - 1) * N:(l - 1) * N + 3] = [0, primes[l - 1] - 1, primes[l - 1] // 2]
    return src, ct_in


def row_stage_one(hg, oracle, rescale, depth):
    c, o, primes = shape(hg, oracle, "A")
    Q = c.Q_size
    l = Q - depth
    src, ct_in = _moddown_inputs(oracle, c, primes, depth)
    want = []
    if not rescale:  # relinearize form: in [2][l+1][N] (limbs 0..l-1 and the special prime), out [2][l][N]
        half, half_mod = o.table("half"), o.table("half_mod")
        for b in range(B):
            w = np.zeros(2 * l * N, dtype=np.uint64)
            o.L.o_divide_round_lastq_leveled_stage_one(src[b].ctypes.data, w.ctypes.data, o.qp_mods, half.ctypes.data,
                                                       half_mod.ctypes.data, 12, Q, l)
            want.append(w)
        ops = {"src": (src, "in"), "out": (_outs(2 * l * N), "out")}
    else:            # rescale form: [2][l][N] -> [2][l-1][N]
        loc = _rescale_location(Q, depth)
        rhalf, rhm = o.table("rescaled_half"), o.table("rescaled_half_mod")
        for b in range(B):
            w = np.zeros(2 * (l - 1) * N, dtype=np.uint64)
            o.L.o_divide_round_lastq_leveled_stage_one(ct_in[b].ctypes.data, w.ctypes.data, o.qp_mods,
                                                       rhalf.ctypes.data + 8 * depth, rhm.ctypes.data + 8 * loc, 12, l - 1,
                                                       l - 1)
            want.append(w)
        ops = {"src": (ct_in, "in"), "out": (_outs(2 * (l - 1) * N), "out")}
    call = lambda d, s: c.divide_round_lastq_leveled_stage_one(d["src"], s["src"], d["out"], s["out"], rescale, depth, B)
    return ops, call, {"out": want}


def row_stage_two(hg, oracle, sk, depth):
    c, o, primes = shape(hg, oracle, "A")
    l = c.Q_size - depth
    src, _ = _moddown_inputs(oracle, c, primes, depth)
    last = [_limbs(oracle, primes, list(range(l)) * 2, N, 15 + b) for b in range(B)]
    cts = [synth_ct(primes, range(l), 2, N, 70 + b) for b in range(B)]
    inv = o.table("last_q_modinv")
    want = []
    for b in range(B):
        w = np.zeros(2 * l * N, dtype=np.uint64)
        o.L.o_divide_round_lastq_leveled_stage_two(last[b].ctypes.data, src[b].ctypes.data, cts[b].ctypes.data,
                                                   w.ctypes.data, o.qp_mods, inv.ctypes.data, 12, l, sk)
        want.append(w)
    ops = {"last": (last, "in"), "src": (src, "in"), "ct": (cts, "in"), "out": (_outs(2 * l * N), "out")}
    call = lambda d, s: c.divide_round_lastq_leveled_stage_two(d["last"], s["last"], d["src"], s["src"], d["ct"], s["ct"],
                                                               d["out"], s["out"], sk, depth, B)
    return ops, call, {"out": want}


def row_move(hg, oracle, depth):
    c, o, primes = shape(hg, oracle, "A")
    l = c.Q_size - depth
    _, ct_in = _moddown_inputs(oracle, c, primes, depth)
    want = []
    for b in range(B):
        w = np.full(2 * l * N, 7, dtype=np.uint64)  # the dropped limb's slot stays untouched
        o.L.o_move_cipher_leveled(ct_in[b].ctypes.data, w.ctypes.data, 12, l - 1)
        want.append(w)
    ops = {"src": (ct_in, "in"), "out": (_outs(2 * l * N), "out")}
    call = lambda d, s: c.move_cipher_leveled(d["src"], s["src"], d["out"], s["out"], depth, B)
    return ops, call, {"out": want}


def row_rescale_divide(hg, oracle, depth):
    c, o, primes = shape(hg, oracle, "A")
    Q = c.Q_size
    l = Q - depth
    loc = _rescale_location(Q, depth)
    rinv = o.table("rescaled_last_q_modinv")
    _, ct_in = _moddown_inputs(oracle, c, primes, depth)
    last = [_limbs(oracle, primes, list(range(l - 1)) * 2, N, 25 + b) for b in range(B)]
    want = []
    for b in range(B):
        w = np.zeros(2 * (l - 1) * N, dtype=np.uint64)
        o.L.o_divide_round_lastq_rescale(last[b].ctypes.data, ct_in[b].ctypes.data, w.ctypes.data, o.qp_mods,
                                         rinv.ctypes.data + 8 * loc, 12, l - 1)
        want.append(w)
    ops = {"last": (last, "in"), "src": (ct_in, "in"), "out": (_outs(2 * (l - 1) * N), "out")}
    call = lambda d, s: c.divide_round_lastq_rescale(d["last"], s["last"], d["src"], s["src"], d["out"], s["out"], depth, B)
    return ops, call, {"out": want}


def row_extended(hg, oracle, mode, depth):
    c, o, primes = shape(hg, oracle, "B")
    Q, Qp = c.Q_size, c.Q_prime_size
    l, rc = Q - depth, Qp - depth
    ids = list(range(l)) + list(range(Q, Qp))
    src = [_limbs(oracle, primes, ids * 2, N, 33 + b) for b in range(B)]
    for s_ in src:
        s_[l * N:l * N + 3] = [0, primes[Q] - 1, primes[Q] // 2]
    cts = [synth_ct(primes, range(l), 2, N, 44 + b) for b in range(B)]
    want = []
    for b in range(B):
        w = np.zeros(2 * l * N, dtype=np.uint64)
        o.L.o_divide_round_lastq_extended(o.h, src[b].ctypes.data, cts[b].ctypes.data, w.ctypes.data, rc, l, mode)
        want.append(w)
    ops = {"src": (src, "in"), "ct": (cts, "in"), "out": (_outs(2 * l * N), "out")}
    call = lambda d, s: c.divide_round_lastq_extended(d["src"], s["src"], d["ct"], s["ct"], d["out"], s["out"], mode, depth, B)
    return ops, call, {"out": want}


def row_mod_raise(hg, oracle):
    c, o, primes = shape(hg, oracle, "A")
    Q = c.Q_size
    v = planted(primes[:Q], 2, B, N, 17)
    want = want_raise(v, primes[:Q], Q).reshape(B, 2 * Q * N)
    ops = {"src": ([v[b].reshape(-1) for b in range(B)], "in"), "out": (_outs(2 * Q * N), "out")}
    call = lambda d, s: c.mod_raise(d["src"], s["src"], d["out"], s["out"], Q, 2, B)
    return ops, call, {"out": list(want)}


def row_fast_convertion(hg, oracle):
    c, o, primes = shape(hg, oracle, "C")
    Q, L = c.Q_size, len(c.table("q_Bsk_merge_modulus"))
    ct1 = [synth_ct(primes, range(Q), 2, N, 1 + b) for b in range(B)]
    ct2 = [synth_ct(primes, range(Q), 2, N, 9 + b) for b in range(B)]
    for x in ct1:
        x[:3] = [0, primes[0] - 1, primes[0] // 2]
    want = []
    for b in range(B):
        w = np.zeros(4 * L * N, dtype=np.uint64)
        o.L.o_fast_convertion(o.h, ct1[b].ctypes.data, ct2[b].ctypes.data, w.ctypes.data)
        want.append(w)
    ops = {"in1": (ct1, "in"), "in2": (ct2, "in"), "out": (_outs(4 * L * N), "out")}
    call = lambda d, s: c.fast_convertion(d["in1"], s["in1"], d["in2"], s["in2"], d["out"], s["out"], B)
    return ops, call, {"out": want}


def row_fast_floor(hg, oracle):
    c, o, primes = shape(hg, oracle, "C")
    Q = c.Q_size
    mm = [int(v) for v in c.table("q_Bsk_merge_modulus")]
    L = len(mm)
    src = [_limbs(oracle, mm, list(range(L)) * 3, N, 33 + b) for b in range(B)]
    for s_ in src:
        s_[Q * N:Q * N + 2] = [0, mm[Q] - 1]
    want = []
    for b in range(B):
        w = np.zeros(3 * Q * N, dtype=np.uint64)
        o.L.o_fast_floor(o.h, src[b].ctypes.data, w.ctypes.data)
        want.append(w)
    ops = {"src": (src, "in"), "out": (_outs(3 * Q * N), "out")}
    call = lambda d, s: c.fast_floor(d["src"], s["src"], d["out"], s["out"], B)
    return ops, call, {"out": want}


def row_ckks_multiply(hg, oracle, depth):
    c, o, primes = shape(hg, oracle, "A")
    l = c.Q_size - depth
    ct1 = [synth_ct(primes, range(l), 2, N, 1 + 10 * b) for b in range(B)]
    ct2 = [synth_ct(primes, range(l), 2, N, 2 + 10 * b) for b in range(B)]
    want = [o.ckks_multiply(ct1[b], ct2[b], depth) for b in range(B)]
    ops = {"ct1": (ct1, "in"), "ct2": (ct2, "in"), "out": (_outs(3 * l * N), "out")}
    call = lambda d, s: c.ckks_multiply(d["ct1"], s["ct1"], d["ct2"], s["ct2"], d["out"], s["out"], depth, B)
    return ops, call, {"out": want}


def row_ckks_rescale(hg, oracle, depth):
    c, o, primes = shape(hg, oracle, "A")
    l = c.Q_size - depth
    cts = [synth_ct(primes, range(l), 2, N, 3 + 10 * b) for b in range(B)]
    want = [o.ckks_rescale(x.copy(), depth)[:2 * (l - 1) * N] for x in cts]
    ops = {"ct": (cts, "inout"), "ws": _ws(c, hg.OP_CKKS_RESCALE, depth, B)}
    call = lambda d, s: c.ckks_rescale_inplace(d["ct"], s["ct"], depth, B, d["ws"])
    return ops, call, {"ct": want}


FLAT = ("packed", "off8")  # entries whose pointers carry no stride
ROWS = {
    "addition_add": (lambda hg, o: row_addition(hg, o, 0), FLAT),
    "addition_sub": (lambda hg, o: row_addition(hg, o, 1), FLAT),
    "addition_neg": (lambda hg, o: row_addition(hg, o, 2), FLAT),
    "cross_multiplication_qp": (lambda hg, o: row_cross_multiplication(hg, o, False), tuple(LAYOUTS)),
    "cross_multiplication_q_bsk": (lambda hg, o: row_cross_multiplication(hg, o, True), tuple(LAYOUTS)),
    "cipher_broadcast": (lambda hg, o: row_cipher_broadcast(hg, o, False), tuple(LAYOUTS)),
    "cipher_broadcast_leveled": (lambda hg, o: row_cipher_broadcast(hg, o, True), tuple(LAYOUTS)),
    "keyswitch_multiply_accumulate": (lambda hg, o: row_keyswitch_mac(hg, o, False), tuple(LAYOUTS)),
    "keyswitch_multiply_accumulate_leveled": (lambda hg, o: row_keyswitch_mac(hg, o, True), tuple(LAYOUTS)),
    "base_conversion_DtoQtilde_depth0": (lambda hg, o: row_base_conversion(hg, o, 0), tuple(LAYOUTS)),
    "base_conversion_DtoQtilde_depth1": (lambda hg, o: row_base_conversion(hg, o, 1), tuple(LAYOUTS)),
    "divide_round_lastq_switchkey0": (lambda hg, o: row_divide_round_lastq(hg, o, 0), tuple(LAYOUTS)),
    "divide_round_lastq_switchkey1": (lambda hg, o: row_divide_round_lastq(hg, o, 1), tuple(LAYOUTS)),
    "divide_round_lastq_permute_bfv": (lambda hg, o: row_permute(hg, o, "C", 0), tuple(LAYOUTS)),
    "divide_round_lastq_permute_ckks": (lambda hg, o: row_permute(hg, o, "A", 1), tuple(LAYOUTS)),
    "divide_round_lastq_permute_two_special": (lambda hg, o: row_permute(hg, o, "B", 0), tuple(LAYOUTS)),
    "leveled_stage_one_depth0": (lambda hg, o: row_stage_one(hg, o, 0, 0), tuple(LAYOUTS)),
    "leveled_stage_one_depth1": (lambda hg, o: row_stage_one(hg, o, 0, 1), tuple(LAYOUTS)),
    "leveled_stage_one_rescale_depth0": (lambda hg, o: row_stage_one(hg, o, 1, 0), tuple(LAYOUTS)),
    "leveled_stage_one_rescale_depth1": (lambda hg, o: row_stage_one(hg, o, 1, 1), tuple(LAYOUTS)),
    "leveled_stage_two_switchkey0": (lambda hg, o: row_stage_two(hg, o, 0, 1), tuple(LAYOUTS)),
    "leveled_stage_two_switchkey1": (lambda hg, o: row_stage_two(hg, o, 1, 0), tuple(LAYOUTS)),
    "move_cipher_leveled_depth0": (lambda hg, o: row_move(hg, o, 0), tuple(LAYOUTS)),
    "move_cipher_leveled_depth1": (lambda hg, o: row_move(hg, o, 1), tuple(LAYOUTS)),
    "divide_round_lastq_rescale_depth0": (lambda hg, o: row_rescale_divide(hg, o, 0), tuple(LAYOUTS)),
    "divide_round_lastq_rescale_depth1": (lambda hg, o: row_rescale_divide(hg, o, 1), tuple(LAYOUTS)),
    "divide_round_lastq_extended_mode0": (lambda hg, o: row_extended(hg, o, 0, 0), tuple(LAYOUTS)),
    "divide_round_lastq_extended_mode1": (lambda hg, o: row_extended(hg, o, 1, 1), tuple(LAYOUTS)),
    "divide_round_lastq_extended_mode2": (lambda hg, o: row_extended(hg, o, 2, 0), tuple(LAYOUTS)),
    "mod_raise": (row_mod_raise, tuple(LAYOUTS)),
    "fast_convertion": (row_fast_convertion, tuple(LAYOUTS)),
    "fast_floor": (row_fast_floor, tuple(LAYOUTS)),
    "ckks_multiply_depth0": (lambda hg, o: row_ckks_multiply(hg, o, 0), tuple(LAYOUTS)),
    "ckks_multiply_depth1": (lambda hg, o: row_ckks_multiply(hg, o, 1), tuple(LAYOUTS)),
    "ckks_rescale_inplace_depth0": (lambda hg, o: row_ckks_rescale(hg, o, 0), tuple(LAYOUTS)),
    "ckks_rescale_inplace_depth1": (lambda hg, o: row_ckks_rescale(hg, o, 1), tuple(LAYOUTS)),
}
_rows = {}


@pytest.mark.parametrize("row,layout", [(r, lay) for r, (_, lays) in ROWS.items() for lay in lays])
def test_streaming_entry(hg, oracle, torch, row, layout):
    """the oracle's residues, every sentinel intact, inputs unchanged -- in each layout, shared by every operand"""
    if row not in _rows:
        _rows[row] = ROWS[row][0](hg, oracle)
    operands, call, want = _rows[row]
    got = _run(torch, operands, lambda name: LAYOUTS[layout], call)
    _compare(got, want, (row, layout))


# ------------------------------------------------------------------ (c) key switch, every role and every form
HOISTED_STEPS = [0, 1, -2, 5, None, 3, 0, -1]  # None: the conjugation; six keys: a group of four and a group of two


def _forms(hg, call):
    """(natural, wide, split) launches of the fused row pass made by call()"""
    before = hg.ks_launch_forms()
    call()
    return tuple(b - a for a, b in zip(before, hg.ks_launch_forms()))


def _row_launches(which, entry):
    """the fused row-pass launches of one forced call: per launch the roles whose operands it moves in pairs"""
    if entry.startswith("hoisted"):
        return []
    if which in ("A", "D"):
        return [{"key", "ws", "ct"}, {"key", "ct", "out"}]
    return [{"key", "ws"}]


def _placements(roles):
    """name -> role -> (lead, pad): the control, one role at a time 8 bytes off, every operand in the odd layouts"""
    out = {"packed": {r: (0, 0) for r in roles}}
    for r in roles:
        out[r + "_off8"] = {k: (1 if k == r else 0, 0) for k in roles}
    out["odd"] = {r: LAYOUTS["odd"] for r in roles}
    out["off8_odd"] = {r: LAYOUTS["off8_odd"] for r in roles}
    return out


def _bad_roles(place):
    """roles with an operand 8 bytes off, or with an odd item stride (the key and the workspace carry no stride)"""
    return {r for r, (lead, pad) in place.items() if lead or (pad % 2 and r in ("ct", "out"))}


_ks_cases = {}


def _ks_case(hg, oracle, which, entry, depth, batch=B):
    """(operands: name -> (items, kind, role), call, want) of one key-switch entry, made once"""
    tag = (which, entry, depth)
    if tag in _ks_cases:
        return _ks_cases[tag]
    c, o, primes = shape(hg, oracle, which)
    n = c.n
    Q, Qp, P = c.Q_size, c.Q_prime_size, c.P_size
    bfv = which == "C"
    l = Q - depth
    digits = Q if P == 1 else -(-Q // P)
    words = 2 * l * n
    if entry == "relinearize":
        key = synth_key(primes, digits, Qp, n, 3)
        cts = [synth_ct(primes, range(l), 3, n, 1 + 10 * b) for b in range(batch)]
        fn = o.bfv_relinearize if bfv else (o.ckks_relinearize if P == 1 else o.ckks_relinearize_II)
        want = [(fn(x.copy(), key) if bfv else fn(x.copy(), key, depth))[:words] for x in cts]
        op = hg.OP_BFV_RELIN if bfv else hg.OP_CKKS_RELIN
        operands = {"ct": (cts, "inout", "ct"), "key": ([key], "in", "key"), "ws": _ws(c, op, depth, batch) + ("ws",)}
        if bfv:
            call = lambda d, s: c.bfv_relinearize_inplace(d["ct"], s["ct"], d["key"], batch, d["ws"])
        else:
            call = lambda d, s: c.ckks_relinearize_inplace(d["ct"], s["ct"], d["key"], depth, batch, d["ws"])
        case = (operands, call, {"ct": want})
    elif entry.startswith("galois"):
        step = entry[len("galois_"):]
        if bfv:
            g = hg.steps_to_galois_elt(1, n, 3)
        else:
            g = 2 * n - 1 if step == "conj" else hg.steps_to_galois_elt(int(step), n, 5)
        key = synth_key(primes, digits, Qp, n, 5)
        cts = [synth_ct(primes, range(l), 2, n, 1 + 10 * b) for b in range(batch)]
        if bfv:
            want = [o.bfv_apply_galois(x, key, g) for x in cts]
        else:
            fn = o.ckks_apply_galois if P == 1 else o.ckks_apply_galois_II
            want = [fn(x, key, g, depth) for x in cts]
        op = hg.OP_BFV_GALOIS if bfv else hg.OP_CKKS_GALOIS
        operands = {"ct": (cts, "in", "ct"), "out": (_outs(words, batch), "out", "out"), "key": ([key], "in", "key"),
                    "ws": _ws(c, op, depth, batch) + ("ws",)}
        if bfv:
            call = lambda d, s: c.bfv_apply_galois(d["ct"], s["ct"], d["out"], s["out"], d["key"], g, batch, d["ws"])
        else:
            call = lambda d, s: c.ckks_apply_galois(d["ct"], s["ct"], d["out"], s["out"], d["key"], g, depth, batch, d["ws"])
        case = (operands, call, {"out": want})
    else:  # hoisted4: the OP_CKKS_ROTATE_HOISTED workspace (four accumulators), hoisted1: the OP_CKKS_GALOIS one
        elts = [0 if st == 0 else 2 * n - 1 if st is None else hg.steps_to_galois_elt(st, n, 5) for st in HOISTED_STEPS]
        keys = [None if g == 0 else synth_key(primes, digits, Qp, n, 20 + i) for i, g in enumerate(elts)]
        cts = [synth_ct(primes, range(l), 2, n, 5 + b) for b in range(batch)]
        want = [o.ckks_rotate_hoisted(x, keys, elts, depth) for x in cts]
        op = hg.OP_CKKS_ROTATE_HOISTED if entry == "hoisted4" else hg.OP_CKKS_GALOIS
        operands = {"ct": (cts, "in", "ct"), "out": (_outs(len(elts) * words, batch), "out", "out"),
                    "ws": _ws(c, op, depth, batch) + ("ws",)}
        for i, k in enumerate(keys):
            if k is not None:
                operands["key%d" % i] = ([k], "in", "key")
        call = lambda d, s: c.ckks_rotate_hoisted(d["ct"], s["ct"], d["out"], s["out"], [d.get("key%d" % i) for i in range(len(elts))],
                                                  elts, depth, batch, d["ws"])
        case = (operands, call, {"out": want})
    _ks_cases[tag] = case
    return case


def _key_switch(hg, oracle, torch, which, entry, depth, setting, batch=B, only=None):
    c = shape(hg, oracle, which)[0]
    operands, call, want = _ks_case(hg, oracle, which, entry, depth, batch)
    plain = {name: (items, kind) for name, (items, kind, _) in operands.items()}
    role = {name: r for name, (_, _, r) in operands.items()}
    roles = [r for r in ("ct", "out", "key", "ws") if r in role.values()]
    launches = _row_launches(which, entry)
    for k, v in SETTINGS[setting].items():
        c.set_option(k, v)
    try:
        seen = {}
        for pname, place in _placements(roles).items():
            if only and pname not in only:
                continue
            box = {}
            forms = _forms(hg, lambda: box.update(_run(torch, plain, lambda name: place[role[name]], call)))
            print(which, entry, depth, setting, pname, "forms (natural, wide, split):", forms)
            _compare(box, want, (which, entry, depth, setting, pname))
            seen[pname] = forms
            if setting.startswith("forced"):
                natural = sum(1 for roles_of in launches if roles_of & _bad_roles(place))
                assert forms == (natural, len(launches) - natural, 0), (pname, forms)
        if setting.startswith("forced"):
            assert seen["packed"] == (0, len(launches), 0)
            for pname, (nat, wide, _) in seen.items():  # as many launches as the control made wide ones
                assert nat + wide == seen["packed"][1], (pname, seen)
        if setting == "split2":
            # the only launches of ks_row_mac_split and rns_sum_partials on such operands
            assert all(f[0] == 0 and f[1] == 0 and f[2] > 0 for f in seen.values()), seen
    finally:
        for k, v in SETTINGS["default"].items():
            c.set_option(k, v)


KS_ENTRIES = ["relinearize", "galois_1", "galois_-3", "galois_conj", "hoisted4", "hoisted1"]
KS_CASES = [(w, e, d, s) for w in ("A", "B") for e in KS_ENTRIES for d in (0, 1)
            for s in ("default", "forced_col0", "forced_col1")]
# digit splits need four digits: shape A at depth 0
KS_CASES += [("A", e, 0, "split2") for e in ("relinearize", "galois_1", "galois_-3", "galois_conj")]
KS_CASES += [("C", e, 0, s) for e in ("relinearize", "galois_1") for s in ("default", "forced_col0", "forced_col1")]


@pytest.mark.parametrize("which,entry,depth,setting", KS_CASES)
def test_key_switch_roles_and_forms(hg, oracle, torch, which, entry, depth, setting):
    """one role at a time 8 bytes off, then everything in the odd layouts: the oracle's residues, sentinels intact, and
    under the forced fused path the launch forms that the operands of each launch call for"""
    _key_switch(hg, oracle, torch, which, entry, depth, setting)


# ------------------------------------------------------------------ (d) N = 2^15, the forced fused path
@pytest.mark.parametrize("entry", ["relinearize", "galois_1"])
def test_two_pass_degree_forced_fused(hg, oracle, torch, entry):
    """two-pass transforms, the row kernels walk eight tiles; depth 1 keeps the oracle at three limbs per part"""
    _key_switch(hg, oracle, torch, "D", entry, 1, "forced_col1", batch=2, only=("packed", "off8_odd"))


# ------------------------------------------------------------------ (e) extremes through the natural kernels
def test_extreme_values_through_the_natural_kernels(hg, oracle, torch):
    """every residue q - 1, alternating 0 / q - 1 (in the NTT and in the coefficient domain) against a key of all q - 1,
    every operand 8 bytes off: the natural kernels only, and the oracle's residues"""
    c, o, primes = shape(hg, oracle, "A")
    Q, Qp = c.Q_size, c.Q_prime_size
    pats = ["max", "alt", "alt_coeff"]
    key = np.concatenate([np.full(N, primes[j] - 1, dtype=np.uint64) for _ in range(Q) for _c in range(2) for j in range(Qp)])
    cts = [np.concatenate([extreme_limbs(c, primes, range(Q), N, pat, 31 * i + p) for p in range(3)]) for i, pat in enumerate(pats)]
    want = [o.ckks_relinearize(x.copy(), key, 0)[:2 * Q * N] for x in cts]
    operands = {"ct": (cts, "inout"), "key": ([key], "in"), "ws": _ws(c, hg.OP_CKKS_RELIN, 0, len(cts))}
    call = lambda d, s: c.ckks_relinearize_inplace(d["ct"], s["ct"], d["key"], 0, len(cts), d["ws"])
    for k, v in SETTINGS["forced_col1"].items():
        c.set_option(k, v)
    try:
        box = {}
        forms = _forms(hg, lambda: box.update(_run(torch, operands, lambda name: LAYOUTS["off8"], call)))
    finally:
        for k, v in SETTINGS["default"].items():
            c.set_option(k, v)
    assert forms[0] > 0 and forms[1] == 0 and forms[2] == 0, forms
    _compare(box, {"ct": want}, "extremes")


# ------------------------------------------------------------------ (b) one-pass leaves
# Each leaf in the control layout and with every operand 8 bytes off on odd strides, compared as its own test file compares
# it: the Python-integer models of tests/test_gpu_linear_transform.py, test_gpu_poly_eval.py and test_gpu_logic.py, the
# chains of single entries (run on packed copies) of test_gpu_poly_eval.py, test_gpu_logic.py and
# test_gpu_encoding_transform.py.  Diagonals and plaintext operands get the same lead as the ciphertexts.
LEAF_LAYOUTS = ("packed", "off8_odd")
_leaves = {}


def _leaf(name, build):
    if name not in _leaves:
        _leaves[name] = build()
    return _leaves[name]


def _leaf_run(torch, name, build, layout):
    operands, call, want = _leaf(name, build)
    got = _run(torch, operands, lambda _: LAYOUTS[layout], call)
    _compare(got, want, (name, layout))


@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_diag_mac(hg, torch, layout):
    from test_gpu_linear_transform import _want_diag_mac
    from test_gpu_poly_eval import context

    def build():
        c, primes = context(hg, [60, 60, 60], [60])
        l, index, n_diag = 3, [[0, 1, 2], [3, -1, 4], [-1, -1, -1]], 5  # full, with a hole, entirely absent (zeros)
        n1, n2, words = 3, 3, 2 * 3 * N
        rot = [np.stack([synth_ct(primes, range(l), 2, N, 40 + 100 * b + i).reshape(2, l, N) for i in range(n1)]) for b in range(B)]
        diags = np.stack([synth_ct(primes, range(l), 1, N, 900 + d).reshape(l, N) for d in range(n_diag)])
        want = [_want_diag_mac(rot[b], diags, index, primes, l).reshape(-1) for b in range(B)]
        operands = {"rot": ([r.reshape(-1) for r in rot], "in"), "diags": ([diags.reshape(-1)], "in"),
                    "out": (_outs(n2 * words), "out")}
        call = lambda d, s: c.ckks_diag_mac(d["rot"], s["rot"], n1, d["diags"], n_diag, index, n2, d["out"], s["out"], 0, B)
        return operands, call, {"out": want}
    _leaf_run(torch, "diag_mac", build, layout)


@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_weighted_sum(hg, torch, layout):
    from test_gpu_poly_eval import context, weighted_sum_model

    def build():
        c, primes = context(hg, [60, 40, 40, 40, 40], [60])
        psi_half = c.table("psi_half")
        limbs, term_limbs = 3, [3, 5, 3]
        rng = np.random.default_rng(31)
        terms = [[synth_ct(primes, range(L), 2, N, 77 + 10 * i + b) for b in range(B)] for i, L in enumerate(term_limbs)]
        weights = [complex(a, b) for a, b in zip(rng.integers(-2 ** 40, 2 ** 40, 3), rng.integers(-2 ** 40, 2 ** 40, 3))]
        w0 = complex(float(2 ** 80 + 12345 * 2 ** 30), -float(2 ** 41 + 1))
        want = [weighted_sum_model([t[b] for t in terms], term_limbs, weights, w0, limbs, primes, psi_half).reshape(-1)
                for b in range(B)]
        operands = {"t%d" % i: (t, "in") for i, t in enumerate(terms)}
        operands["out"] = (_outs(2 * limbs * N), "out")
        call = lambda d, s: c.ckks_weighted_sum([d["t%d" % i] for i in range(3)], [s["t%d" % i] for i in range(3)], term_limbs,
                                                weights, w0, d["out"], s["out"], limbs, batch=B)
        return operands, call, {"out": want}
    _leaf_run(torch, "weighted_sum", build, layout)


@pytest.mark.parametrize("form", ["ciphertext_higher", "constant"])
@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_double_sub(hg, torch, layout, form):
    from test_gpu_poly_eval import context, drop

    def build():
        c, primes = context(hg, [60, 40, 40, 40, 40], [60])
        limbs, a_limbs, b_limbs = 3, 4, 5
        words = 2 * limbs * N
        with_b = form == "ciphertext_higher"
        value = 0.0 if with_b else 2.0 ** 40 + 0.5
        a = [synth_ct(primes, range(a_limbs), 2, N, 40 + b) for b in range(B)]
        b_ct = [synth_ct(primes, range(b_limbs), 2, N, 50 + b) for b in range(B)]
        # the chain: addition(a, a) then a subtraction, or constant_op (subtract)
        a2 = drop(hg.to_device(np.concatenate(a)), B, a_limbs, limbs)
        c.addition(a2, a2, a2, limbs, 2, B)
        if with_b:
            c.addition(a2, drop(hg.to_device(np.concatenate(b_ct)), B, b_limbs, limbs), a2, limbs, 2, B, op=1)
        else:
            for b in range(B):
                c.ckks_constant_op(1, a2[b * words:], value, limbs, 2, out=a2[b * words:])
        torch.cuda.synchronize()
        want = list(hg.to_host(a2).reshape(B, words))
        operands = {"a": (a, "in"), "out": (_outs(words), "out")}
        if with_b:
            operands["b"] = (b_ct, "in")
        call = lambda d, s: c.ckks_double_sub(d["a"], s["a"], a_limbs, d.get("b"), s["b"] if with_b else 0, b_limbs if with_b else 0,
                                              value, d["out"], s["out"], limbs, batch=B)
        return operands, call, {"out": want}
    _leaf_run(torch, "double_sub_" + form, build, layout)


@pytest.mark.parametrize("gate,kind", [("XNOR", 1), ("XNOR", 2), ("NOT", 0)], ids=["xnor_cipher", "xnor_plain", "not"])
@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_ckks_gate_combine(hg, torch, layout, gate, kind):
    from test_gpu_logic import BIG_ONE, context, gate_id, model

    def build():
        c, primes = context(hg, hg.CKKS, [60, 40, 40, 40, 40], [60])
        limbs = 3
        a_limbs, b_limbs, p_limbs = limbs + 1, limbs + 2, limbs
        a = [synth_ct(primes, range(a_limbs), 2, N, 503 + i) for i in range(B)]
        bh = [synth_ct(primes, range(b_limbs), 2 if kind == 1 else 1, N, 513 + 10 * kind + i) for i in range(B)]
        p = [synth_ct(primes, range(p_limbs), 2, N, 533 + i) for i in range(B)]
        one_int = int(round(BIG_ONE))
        want = []
        for i in range(B):
            res = np.zeros((2, limbs, N), dtype=np.uint64)
            for z in range(2):
                for j in range(limbs):
                    q = primes[j]
                    bj = None
                    if kind == 1:
                        bj = bh[i].reshape(2, b_limbs, N)[z, j]
                    elif kind == 2 and z == 0:
                        bj = bh[i].reshape(b_limbs, N)[j]
                    res[z, j] = model(gate, a[i].reshape(2, a_limbs, N)[z, j], bj, p[i].reshape(2, p_limbs, N)[z, j],
                                      one_int % q if z == 0 else None, q)
            want.append(res.reshape(-1))
        operands = {"a": (a, "in"), "out": (_outs(2 * limbs * N), "out")}
        if kind:
            operands["b"] = (bh, "in")
        if gate != "NOT":
            operands["p"] = (p, "in")
        no_p = gate == "NOT"
        call = lambda d, s: c.ckks_gate_combine(gate_id(hg, gate), d["a"], s["a"], a_limbs, d.get("b"), kind, s["b"] if kind else 0,
                                                b_limbs if kind else 0, d.get("p"), 0 if no_p else s["p"], 0 if no_p else p_limbs,
                                                BIG_ONE, d["out"], s["out"], limbs, batch=B)
        return operands, call, {"out": want}
    _leaf_run(torch, "ckks_gate_combine_%s_%d" % (gate, kind), build, layout)


@pytest.mark.parametrize("gate,kind", [("XNOR", 1), ("XNOR", 2), ("NOT", 0)], ids=["xnor_cipher", "xnor_plain", "not"])
@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_bfv_gate_combine(hg, torch, layout, gate, kind):
    from test_gpu_logic import BFV_SETS, T, bfv_scaled, chain_tail, context, gate_id, model

    def build():
        c, primes = context(hg, hg.BFV, *BFV_SETS["method_I"])
        Q = c.Q_size
        words = 2 * Q * N
        cd = [int(x) for x in c.table("coeff_div_plain_modulus")]
        q_mod_t, thr = int(c.table("Q_mod_t")[0]), int(c.table("upper_threshold")[0])
        rng = np.random.default_rng(9)
        a = [synth_ct(primes, range(Q), 2, N, 700 + i) for i in range(B)]
        bc = [synth_ct(primes, range(Q), 2, N, 710 + i) for i in range(B)]
        bp = [rng.integers(0, T, N).astype(np.uint64) for _ in range(B)]
        bp[0][:3] = [0, 1, T - 1]
        p = [synth_ct(primes, range(Q), 2, N, 720 + i) for i in range(B)]
        bh = {0: None, 1: bc, 2: bp}[kind]
        ca, cp = hg.to_device(np.concatenate(a)), hg.to_device(np.concatenate(p))
        cb = None if bh is None else hg.to_device(np.concatenate(bh))
        chain = chain_tail(c, hg, torch, True, gate, ca, cb, kind, cp, Q, B, 0.0)
        torch.cuda.synchronize()
        want = list(hg.to_host(chain).reshape(B, words))
        one = np.zeros(N, dtype=np.uint64)
        for i in range(B):  # the chain's result is the Python-integer model's
            res = want[i].reshape(2, Q, N)
            for z in range(2):
                for j in range(Q):
                    bj = None
                    if kind == 1:
                        bj = bc[i].reshape(2, Q, N)[z, j]
                    elif kind == 2 and z == 0:
                        bj = np.array(bfv_scaled(bp[i], j, primes, cd, q_mod_t, thr), dtype=np.uint64)
                    one[0] = bfv_scaled([1], j, primes, cd, q_mod_t, thr)[0]
                    m = model(gate, a[i].reshape(2, Q, N)[z, j], bj, p[i].reshape(2, Q, N)[z, j],
                              one.astype(object) if z == 0 else None, primes[j])
                    assert np.array_equal(res[z, j], m), (gate, kind, i, z, j)
        operands = {"a": (a, "in"), "out": (_outs(words), "out")}
        if kind:
            operands["b"] = (bh, "in")
        if gate != "NOT":
            operands["p"] = (p, "in")
        call = lambda d, s: c.bfv_gate_combine(gate_id(hg, gate), d["a"], s["a"], d.get("b"), kind, s["b"] if kind else 0,
                                               d.get("p"), s["p"] if gate != "NOT" else 0, d["out"], s["out"], batch=B)
        return operands, call, {"out": want}
    _leaf_run(torch, "bfv_gate_combine_%s_%d" % (gate, kind), build, layout)


@pytest.mark.parametrize("entry", ["split", "merge"])
@pytest.mark.parametrize("layout", LEAF_LAYOUTS)
def test_leaf_conj_split_and_merge(hg, torch, layout, entry):
    from test_gpu_poly_eval import context

    def build():
        c, primes = context(hg, [60, 60, 60], [60])
        Q, l, dropped = c.Q_size, 3, 1
        depth, out_depth, lo = Q - l, Q - l + dropped, l - dropped
        xs = [synth_ct(primes, range(l), 2, N, 10 + b) for b in range(B)]
        ys = [synth_ct(primes, range(l), 2, N, 20 + b) for b in range(B)]
        want = {"out0": [], "out1": [], "merged": []}
        for b in range(B):  # the composition of single entries on the kept limbs of both parts
            a = hg.to_device(np.ascontiguousarray(xs[b].reshape(2, l, N)[:, :lo]).reshape(-1))
            k = hg.to_device(np.ascontiguousarray(ys[b].reshape(2, l, N)[:, :lo]).reshape(-1))
            s_, d_ = torch.empty_like(a), torch.empty_like(a)
            c.addition(a, k, s_, lo, 2, 1, op=0)
            c.addition(a, k, d_, lo, 2, 1, op=1)
            d_ = c.ckks_mult_i(d_, lo, 2, divide=True)
            m = torch.empty_like(a)
            c.addition(a, c.ckks_mult_i(k, lo, 2, divide=False), m, lo, 2, 1, op=0)
            torch.cuda.synchronize()
            for name, t in (("out0", s_), ("out1", d_), ("merged", m)):
                want[name].append(hg.to_host(t).copy())
        ow = 2 * lo * N
        operands = {"x": (xs, "in"), "y": (ys, "in")}
        if entry == "split":
            operands.update(out0=(_outs(ow), "out"), out1=(_outs(ow), "out"))
            # one stride for both outputs: they are laid out alike
            call = lambda d, s: c.ckks_conj_split(d["x"], s["x"], d["y"], s["y"], d["out0"], d["out1"], s["out0"], depth, out_depth, B)
            return operands, call, {"out0": want["out0"], "out1": want["out1"]}
        operands["merged"] = (_outs(ow), "out")
        call = lambda d, s: c.ckks_conj_merge(d["x"], s["x"], d["y"], s["y"], d["merged"], s["merged"], depth, out_depth, B)
        return operands, call, {"merged": want["merged"]}
    _leaf_run(torch, "conj_" + entry, build, layout)
