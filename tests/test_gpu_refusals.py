"""GPU: what the entries that upload the context FIRST refuse, as a table of (context, entry, arguments) -> (return code,
exact hegpu_last_error() text), and the empty-batch no-op of every entry that has one.  Nothing is launched: every row is a
refusal or a no-op, and after each the sentinel-filled buffers are unchanged.

Every row would be well-formed and in bounds were it accepted: every pointer is a device buffer larger than any accepted
call of these shapes needs, every host array is real, "workspace too small" is a full-size workspace stated one byte short,
the overlap rows alias inside one buffer, a bad depth is Q (no limb left: nothing to address), a bad Galois element is even
and below 2N, a bad index is one past the packed diagonals, for which the buffer has room.  Null pointers and the grid limit
are not here (an accepted null is a fault, an accepted 65536-item call needs buffers nobody should allocate)."""
import ctypes

import pytest
import torch

import heongpu_amd as hg
from heongpu_amd import _lib

pytestmark = pytest.mark.gpu

N = 4096
Q = 3
SENT = 0x5A5A5A5A5A5A5A5A
INV, LOGIC = hg.E_INVALID, hg.E_LOGIC
ROOM = 1 << 21  # words per buffer: 17 ciphertexts per item, two items
STRIDE = ROOM // 2
W = 2 * Q * N  # a two-part ciphertext at depth 0
TABLES_PLAIN = 2


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.ctx = {"ckks": hg.Context.from_bit_sizes(hg.CKKS, N, [40, 30, 30], [40], sec=hg.SEC_NONE),
             "bfv": hg.Context.from_bit_sizes(hg.BFV, N, [40, 30, 30], [40], plain_modulus=65537, sec=hg.SEC_NONE),
             "ckks2": hg.Context.from_bit_sizes(hg.CKKS, N, [40, 30, 30], [40, 40], sec=hg.SEC_NONE)}
    for c in e.ctx.values():
        c.upload()
    e.X, e.X2, e.Y, e.Y2, e.K, e.WS = (torch.full((ROOM,), SENT, dtype=torch.int64, device="cuda") for _ in range(6))
    e.rng, e.crs = hg.Rng(1), hg.Rng(2)
    return e


def _p(t, words=0):
    return t.data_ptr() + 8 * words


def _rows(e):
    X, X2, Y, Y2, K, WS = e.X, e.X2, e.Y, e.Y2, e.K, e.WS
    x, x2, y, y2, k, ws = (_p(t) for t in (X, X2, Y, Y2, K, WS))
    rng, crs = e.rng._h, e.crs._h
    S = STRIDE
    rows = []

    def need(ctx, op, depth=0, batch=2):
        n = e.ctx[ctx].workspace_bytes(op, depth, batch)
        assert 0 < n <= ROOM * 8
        return n

    def table(entry, ctx, ok, cases):
        for change, want in cases:
            a = dict(ok, **change)
            rows.append((a.pop("ctx", ctx), entry, list(a.values()), want, (entry, change)))

    NEG = (INV, "batch must not be negative")
    DEPTH = (INV, "invalid depth")
    SCHEME = (INV, "context scheme mismatch")
    SMALL = (INV, "workspace too small")
    NOOP = (0, None)

    # ---- the kernel entries
    table("hegpu_ntt", "ckks", dict(table_set=hg.TABLES_QP, src=x, dst=y, inverse=0, batch=2, mod_count=2, mod_offset=0,
                                    mod_order=None, poly_order=None, stream=None), [
        ({"table_set": hg.TABLES_Q_BSK}, (INV, "q|Bsk tables exist only in a BFV context")),
        ({"table_set": 3}, (INV, "no such table set in this context")),
        ({"table_set": TABLES_PLAIN}, (INV, "no such table set in this context")),
        ({"mod_count": 0}, (INV, "modulus range outside the table set")),
        ({"table_set": 3, "mod_count": 0}, (INV, "no such table set in this context")),
    ])
    table("hegpu_addition", "ckks", dict(a=x, b=x2, out=y, limbs=Q, parts=2, batch=2, op=0, stream=None), [
        ({"limbs": 0}, (INV, "bad limbs/op")),
        ({"op": 3}, (INV, "bad limbs/op")),
    ])
    table("hegpu_base_conversion_DtoQtilde", "ckks2", dict(src=x, s_in=S, out=y, s_out=S, depth=0, batch=2, stream=None), [
        ({"ctx": "ckks"}, (LOGIC, "method II tables exist only when P_size > 1")),
        ({"depth": Q}, DEPTH),
        ({"ctx": "ckks", "depth": Q}, (LOGIC, "method II tables exist only when P_size > 1")),
    ])
    table("hegpu_divide_round_lastq", "ckks", dict(src=x, s_in=S, ct=x2, s_ct=S, out=y, s_out=S, switchkey=0, batch=2, stream=None), [
        ({"ctx": "ckks2"}, (LOGIC, "divide_round_lastq needs a single special prime (method I)")),
    ])
    table("hegpu_divide_round_lastq_permute", "bfv", dict(src=x, s_in=S, in2=x2, s_in2=S, out=y, s_out=S, galois_elt=3, depth=0,
                                                          batch=2, stream=None), [
        ({"depth": 1}, (INV, "BFV ciphertexts have no depth")),
    ])
    stages = (INV, "CKKS context required")
    single = (LOGIC, "the leveled stages serve a single special prime (method I)")
    table("hegpu_divide_round_lastq_leveled_stage_one", "ckks", dict(src=x, s_in=S, out=y, s_out=S, rescale=0, depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, stages),
        ({"depth": Q}, DEPTH),
        ({"rescale": 1, "depth": Q - 1}, DEPTH),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ctx": "ckks2"}, single),
        ({"ctx": "bfv", "depth": Q, "batch": -1}, stages),
        ({"depth": Q, "batch": -1}, DEPTH),
        ({"depth": Q, "batch": 0}, DEPTH),
        ({"ctx": "ckks2", "batch": 0}, NOOP),
    ])
    table("hegpu_divide_round_lastq_leveled_stage_two", "ckks", dict(last=x, s_last=S, src=x2, s_in=S, ct=x, s_ct=S, out=y, s_out=S, switchkey=0,
                                                                     depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, stages),
        ({"depth": Q}, DEPTH),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ctx": "ckks2"}, single),
    ])
    table("hegpu_move_cipher_leveled", "ckks", dict(src=x, s_in=S, out=y, s_out=S, depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, stages),
        ({"depth": Q - 1}, DEPTH),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
    ])
    table("hegpu_divide_round_lastq_rescale", "ckks", dict(last=x, s_last=S, src=x2, s_in=S, out=y, s_out=S, depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, stages),
        ({"depth": Q - 1}, DEPTH),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
    ])
    table("hegpu_divide_round_lastq_extended", "ckks", dict(src=x, s_in=S, ct=x2, s_ct=S, out=y, s_out=S, mode=1, depth=0, batch=2, stream=None), [
        ({"mode": 3}, (INV, "mode must be 0, 1 or 2")),
        ({"ctx": "bfv", "depth": 1}, (INV, "BFV ciphertexts have no depth")),
        ({"depth": Q}, DEPTH),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"mode": 3, "depth": Q}, (INV, "mode must be 0, 1 or 2")),
        ({"depth": Q, "batch": 0}, DEPTH),
    ])
    table("hegpu_fast_convertion", "bfv", dict(in1=x, s1=S, in2=x2, s2=S, out=y, so=S, batch=2, stream=None), [
        ({"ctx": "ckks"}, (INV, "BFV context required")),
    ])
    table("hegpu_fast_floor", "bfv", dict(src=x, si=S, out=y, so=S, batch=2, stream=None), [
        ({"ctx": "ckks"}, (INV, "BFV context required")),
    ])

    # ---- the operators
    table("hegpu_ckks_multiply", "ckks", dict(ct1=x, s1=S, ct2=x2, s2=S, out=y, so=S, depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"depth": Q}, DEPTH),
    ])
    relin = need("ckks", hg.OP_CKKS_RELIN)
    ok = dict(ct=y, cs=S, key=k, depth=0, batch=2, ws=ws, ws_bytes=relin, stream=None)
    op_cases = [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"ws_bytes": relin - 1}, SMALL),
        ({"ctx": "bfv", "batch": -1}, SCHEME),
        ({"batch": -1, "depth": Q}, NEG),
        ({"batch": 0, "depth": Q, "ws_bytes": 0}, NOOP),  # the empty batch leaves before the depth is looked at
        ({"depth": Q, "ws_bytes": 0}, DEPTH),
    ]
    table("hegpu_ckks_relinearize_inplace", "ckks", ok, op_cases)
    probe = dict(ct=y, cs=S, key=k, depth=0, batch=2, ws=ws, ws_bytes=relin, phases=1, stream=None)
    table("hegpu_probe_ckks_relinearize", "ckks", probe, op_cases + [
        ({"ctx": "ckks2", "ws_bytes": need("ckks2", hg.OP_CKKS_RELIN)}, (LOGIC, "the phase probe covers key-switching method I")),
        ({"ctx": "ckks2", "ws_bytes": 8}, SMALL),
    ])
    resc = need("ckks", hg.OP_CKKS_RESCALE)
    table("hegpu_ckks_rescale_inplace", "ckks", dict(ct=y, cs=S, depth=0, batch=2, ws=ws, ws_bytes=resc, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"ws_bytes": resc - 1}, SMALL),
        ({"depth": Q - 1}, (LOGIC, "no modulus left to rescale by")),
    ])
    gal = need("ckks", hg.OP_CKKS_GALOIS)
    alias = (INV, "apply_galois: out must not alias ct (the result buffer must not contain the input)")
    odd = (INV, "apply_galois: Galois elements are odd and below 2N")
    table("hegpu_ckks_apply_galois", "ckks", dict(ct=x, cs=S, out=y, so=S, key=k, galois_elt=5, depth=0, batch=2, ws=ws, ws_bytes=gal, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"ws_bytes": gal - 1}, SMALL),
        ({"out": _p(X, W - 1)}, alias),
        ({"out": _p(X, S + W - 1), "so": 0}, alias),  # item 0 of out on item 1 of ct
        ({"galois_elt": 0}, odd),
        ({"galois_elt": 2}, odd),
        ({"ws_bytes": 0, "out": x, "galois_elt": 2}, SMALL),
        ({"out": x, "galois_elt": 2}, alias),
        ({"batch": 0, "out": x, "galois_elt": 2}, NOOP),
    ])
    bgal = need("bfv", hg.OP_BFV_GALOIS)
    table("hegpu_bfv_apply_galois", "bfv", dict(ct=x, cs=S, out=y, so=S, key=k, galois_elt=5, batch=2, ws=ws, ws_bytes=bgal, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": bgal - 1}, SMALL),
        ({"out": _p(X, W - 1)}, alias),
    ])
    bmul = need("bfv", hg.OP_BFV_MULTIPLY)
    table("hegpu_bfv_multiply", "bfv", dict(ct1=x, s1=S, ct2=x2, s2=S, out=y, so=S, batch=2, ws=ws, ws_bytes=bmul, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": bmul - 1}, SMALL),
        ({"batch": -1, "ws_bytes": 0}, NEG),
    ])
    brel = need("bfv", hg.OP_BFV_RELIN)
    table("hegpu_bfv_relinearize_inplace", "bfv", dict(ct=y, cs=S, key=k, batch=2, ws=ws, ws_bytes=brel, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": brel - 1}, SMALL),
    ])

    # ---- hoisted rotations, the diagonal sums, the linear transform and the sequences over it
    keys3 = (ctypes.c_void_p * 3)(k, k, k)
    elts3 = (ctypes.c_int * 3)(5, 25, 0)
    even3 = (ctypes.c_int * 3)(5, 0, 6)
    who = "rotate_hoisted: "
    table("hegpu_ckks_rotate_hoisted", "ckks", dict(ct=x, cs=S, out=y, so=S, keys=keys3, elts=elts3, count=3, depth=0, batch=2, ws=ws,
                                                    ws_bytes=gal, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"ws_bytes": gal - 1}, SMALL),
        ({"count": 0}, (INV, who + "empty element list")),
        ({"so": 3 * W - 1}, (INV, who + "out_stride too small")),
        ({"out": _p(X, W - 1)}, (INV, who + "out must not alias ct (the result buffer must not contain the input)")),
        ({"elts": even3}, (INV, who + "Galois elements are odd and below 2N")),
        ({"count": 0, "so": 0}, (INV, who + "empty element list")),
        ({"so": 3 * W - 1, "out": x, "elts": even3}, (INV, who + "out_stride too small")),
        ({"out": x, "elts": even3}, (INV, who + "out must not alias ct (the result buffer must not contain the input)")),
    ])
    n1, n2, n_diag = 2, 2, 3
    index = (ctypes.c_int * 4)(0, 1, 2, -1)
    past = (ctypes.c_int * 4)(0, 1, 2, 3)  # 3: one past the packed diagonals (the buffer has room for it)
    who = "diag_mac: "
    table("hegpu_ckks_diag_mac", "ckks", dict(rot=x, rot_stride=S, n1=n1, diags=k, n_diag=n_diag, index=index, n2=n2, out=y, out_stride=S,
                                              depth=0, batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"n1": 0}, (INV, who + "n1 and n2 lie in [1, 16] (16 products per 128-bit sum, 256 indices by value)")),
        ({"n2": 0}, (INV, who + "n1 and n2 lie in [1, 16] (16 products per 128-bit sum, 256 indices by value)")),
        ({"n_diag": 0, "index": (ctypes.c_int * 4)(-1, -1, -1, -1)}, (INV, who + "null argument")),
        ({"index": past}, (INV, who + "index outside [-1, n_diag)")),
        ({"out": _p(X, n1 * W - 1)}, (INV, who + "out must not overlap rot")),
        ({"n1": 0, "n_diag": 0}, (INV, who + "n1 and n2 lie in [1, 16] (16 products per 128-bit sum, 256 indices by value)")),
        ({"index": past, "out": x}, (INV, who + "index outside [-1, n_diag)")),
    ])
    bk, gk = (ctypes.c_void_p * n1)(None, k), (ctypes.c_void_p * n2)(None, k)
    be, ge = (ctypes.c_int * n1)(0, 5), (ctypes.c_int * n2)(0, 25)
    ge_even = (ctypes.c_int * n2)(0, 26)
    lt = e.ctx["ckks"].linear_transform_workspace_bytes(n1, n2, 0, 2)
    assert 0 < lt <= ROOM * 8
    who = "linear_transform: "
    table("hegpu_ckks_linear_transform", "ckks", dict(ct=x, cs=S, out=y, so=S, diags=k, n_diag=n_diag, index=index, n1=n1, n2=n2, baby_keys=bk,
                                                      baby_elts=be, giant_keys=gk, giant_elts=ge, depth=0, batch=2, ws=ws, ws_bytes=lt,
                                                      stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"n1": 0}, (INV, who + "n1 and n2 lie in [1, 16]")),
        ({"n_diag": 0, "index": (ctypes.c_int * 4)(-1, -1, -1, -1)}, (INV, who + "null argument")),
        ({"index": past}, (INV, who + "index outside [-1, n_diag)")),
        ({"giant_elts": ge_even}, (INV, who + "Galois elements are odd and below 2N")),
        ({"out": _p(X, W - 1)}, (INV, who + "out must not overlap ct")),
        ({"ws_bytes": lt - 1}, SMALL),
        ({"index": past, "giant_elts": ge_even}, (INV, who + "index outside [-1, n_diag)")),
        ({"giant_elts": ge_even, "out": x, "ws_bytes": 0}, (INV, who + "Galois elements are odd and below 2N")),
        ({"out": x, "ws_bytes": 0}, (INV, who + "out must not overlap ct")),
    ])

    def factor(**change):
        f = (_lib.LinearFactor * 1)()
        a = dict(diags=k, n_diag=n_diag, index=index, n1=n1, n2=n2, baby_keys=bk, baby_elts=be, giant_keys=gk, giant_elts=ge)
        a.update(change)
        for name, v in a.items():
            setattr(f[0], name, v)
        return f

    good = factor()
    wide = factor(n2=17, index=(ctypes.c_int * 34)(*[-1] * 34), giant_keys=(ctypes.c_void_p * 17)(*[k] * 17),
                  giant_elts=(ctypes.c_int * 17)(*[5] * 17))  # real arrays of the 17 rows it names
    et = int(_lib.load().hegpu_ckks_encoding_transform_workspace_bytes(e.ctx["ckks"]._h, good, 1, 0, 2))
    assert 0 < et <= ROOM * 8
    for entry, who, ok in (
            ("hegpu_ckks_coeff_to_slot", "coeff_to_slot", dict(ct=x, cs=S, out0=y, out1=y2, so=S, factors=good, count=1, conj_key=k, depth=0,
                                                              batch=2, ws=ws, ws_bytes=et, stream=None)),
            ("hegpu_ckks_slot_to_coeff", "slot_to_coeff", dict(c0=x, c0_stride=S, c1=x2, c1_stride=S, out=y, so=S, factors=good, count=1, depth=0,
                                                              batch=2, ws=ws, ws_bytes=et, stream=None))):
        levels = (INV, who + ": depth + factors + 1 must stay below Q (one level per factor, one at the real / imaginary boundary)")
        cases = [
            ({"ctx": "bfv"}, SCHEME),
            ({"batch": -1}, NEG),
            ({"batch": 0}, NOOP),
            ({"depth": Q}, DEPTH),
            ({"count": 0}, (INV, who + ": at least one factor")),
            ({"depth": 1}, levels),
            ({"factors": wide}, (INV, who + ": n1 and n2 lie in [1, 16]")),
            ({"factors": factor(n_diag=0, index=(ctypes.c_int * 4)(-1, -1, -1, -1))}, (INV, who + ": null argument in a factor")),
            ({"factors": factor(index=past)}, (INV, who + ": index outside [-1, n_diag)")),
            ({"factors": factor(giant_elts=ge_even)}, (INV, who + ": Galois elements are odd and below 2N")),
            ({"ws_bytes": et - 1}, SMALL),
            ({"batch": 0, "count": 0}, NOOP),
            ({"depth": 1, "factors": wide}, levels),
            ({"factors": factor(index=past, giant_elts=ge_even), "ws_bytes": 0}, (INV, who + ": index outside [-1, n_diag)")),
        ]
        if who == "coeff_to_slot":
            both = (INV, "coeff_to_slot: the outputs must overlap neither ct nor each other")
            cases += [({"out0": _p(X, W - 1)}, both), ({"out1": _p(X, W - 1)}, both), ({"out1": _p(Y, 2 * N - 1)}, both),
                      ({"out1": y, "ws_bytes": 0}, both)]
        else:
            cases += [({"so": 2 * 2 * N - 1}, (INV, "slot_to_coeff: out_stride too small")),
                      ({"out": _p(X, W - 1)}, (INV, "slot_to_coeff: out must not overlap an input")),
                      ({"out": _p(X2, W - 1)}, (INV, "slot_to_coeff: out must not overlap an input")),
                      ({"out": x, "ws_bytes": 0}, (INV, "slot_to_coeff: out must not overlap an input"))]
        table(entry, "ckks", ok, cases)

    # ---- the passes of the polynomial evaluation and the real / imaginary boundary: an empty batch is refused
    # (arrays of 16 terms, so that the row naming 16 reads real entries)
    terms, strides = (ctypes.c_void_p * 16)(*[x, x2] * 8), (ctypes.c_uint64 * 16)(*[S] * 16)
    limbs2, short = (ctypes.c_int * 16)(*[3, 2] * 8), (ctypes.c_int * 16)(*[3, 1] * 8)
    weights = (ctypes.c_double * 32)(*[1.0, 0.0, 2.0, 1.0] * 8)
    nan = (ctypes.c_double * 32)(*[1.0, 0.0, float("nan"), 1.0] * 8)
    who = "weighted_sum: "
    table("hegpu_ckks_weighted_sum", "ckks", dict(terms=terms, strides=strides, term_limbs=limbs2, weights=weights, count=2, w0_re=1.0,
                                                  w0_im=0.0, out=y, out_stride=S, limbs=2, batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": 0}, (INV, who + "batch must be at least 1")),
        ({"batch": -1}, (INV, who + "batch must be at least 1")),
        ({"count": 16}, (INV, who + "at most 15 terms (15 products and a residue per 128-bit sum)")),
        ({"limbs": 0}, (INV, who + "bad limb count")),
        ({"w0_im": float("inf")}, (INV, who + "a weight is not a finite number")),
        ({"term_limbs": short}, (INV, who + "a term has fewer limbs than the sum")),
        ({"weights": nan}, (INV, who + "a weight is not a finite number")),
        ({"out": _p(X2, 2 * 2 * N - 1)}, (INV, who + "out must not overlap a term")),
        ({"batch": 0, "count": 16, "limbs": 0}, (INV, who + "batch must be at least 1")),
        ({"limbs": 0, "w0_re": float("nan")}, (INV, who + "bad limb count")),
    ])
    who = "double_sub: "
    table("hegpu_ckks_double_sub", "ckks", dict(a=x, a_stride=S, a_limbs=3, b=x2, b_stride=S, b_limbs=2, value=0.0, out=y, out_stride=S, limbs=2,
                                                batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": 0}, (INV, who + "batch must be at least 1")),
        ({"limbs": 0}, (INV, who + "bad limb count")),
        ({"a_limbs": 1}, (INV, who + "bad limb count")),
        ({"b_limbs": Q + 1}, (INV, who + "bad limb count")),
        ({"b": None, "value": float("nan")}, (INV, who + "constant out of range")),
        ({"b": None, "value": -3.4e38}, (INV, who + "constant out of range")),
        ({"out": x}, (INV, who + "out is a itself (equal strides and limb counts) or does not overlap it")),
        ({"out": _p(X2, 2 * 2 * N - 1)}, (INV, who + "out must not overlap b")),
        ({"batch": 0, "limbs": 0}, (INV, who + "batch must be at least 1")),
    ])
    table("hegpu_ckks_conj_split", "ckks", dict(x=x, x_stride=S, xc=x2, xc_stride=S, out0=y, out1=y2, out_stride=S, depth=0, out_depth=1, batch=2,
                                                stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": 0}, (INV, "conj_split: batch must be at least 1")),
        ({"out_depth": Q}, (INV, "conj_split: depth <= out_depth < Q")),
        ({"depth": 2}, (INV, "conj_split: depth <= out_depth < Q")),
        ({"out1": _p(X2, W - 1)}, (INV, "conj_split: an output must not overlap an input")),
        ({"out1": _p(Y, 2 * 2 * N - 1)}, (INV, "conj_split: the two outputs must not overlap")),
        ({"batch": 0, "out_depth": Q}, (INV, "conj_split: batch must be at least 1")),
    ])
    table("hegpu_ckks_conj_merge", "ckks", dict(c0=x, c0_stride=S, c1=x2, c1_stride=S, out=y, out_stride=S, depth=0, out_depth=1, batch=2,
                                                stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": 0}, (INV, "conj_merge: batch must be at least 1")),
        ({"out_depth": Q}, (INV, "conj_merge: depth <= out_depth < Q")),
        ({"out": _p(X2, W - 1)}, (INV, "conj_merge: the output must not overlap an input")),
    ])

    # ---- key generation, encryption, encoding
    sec = need("ckks", hg.OP_KEYGEN_SECRET, 0, 1)
    table("hegpu_generate_secret_key", "ckks", dict(rng=rng, hw=N // 2, sk=y, ws=ws, ws_bytes=sec, stream=None), [
        ({"ws_bytes": sec - 1}, SMALL),
        ({"hw": 0}, (INV, "hamming weight has to be in range 0 to ring size")),
        ({"ws_bytes": 0, "hw": 0}, SMALL),
    ])
    swk = need("ckks", hg.OP_KEYGEN_SWITCH, 0, 1)
    table("hegpu_generate_public_key", "ckks", dict(rng=rng, sk=x, pk=y, ws=ws, ws_bytes=need("ckks", hg.OP_KEYGEN_PUBLIC, 0, 1), stream=None), [
        ({"ws_bytes": need("ckks", hg.OP_KEYGEN_PUBLIC, 0, 1) - 1}, SMALL),
    ])
    table("hegpu_generate_relin_key", "ckks", dict(rng=rng, sk=x, rk=y, ws=ws, ws_bytes=swk, stream=None), [({"ws_bytes": swk - 1}, SMALL)])
    table("hegpu_generate_galois_key", "ckks", dict(rng=rng, sk=x, galois_elt=5, gk=y, ws=ws, ws_bytes=swk, stream=None), [
        ({"ws_bytes": swk - 1}, SMALL),
        ({"galois_elt": 0}, (INV, "galois element must be odd and below 2N")),
        ({"galois_elt": 6}, (INV, "galois element must be odd and below 2N")),
        ({"ws_bytes": 0, "galois_elt": 6}, SMALL),
    ])
    enc = need("ckks", hg.OP_CKKS_ENCRYPT, 0, 1)
    table("hegpu_ckks_encrypt", "ckks", dict(rng=rng, pk=x, plain=x2, ct=y, ws=ws, ws_bytes=enc, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"ws_bytes": enc - 1}, SMALL),
    ])
    benc = need("bfv", hg.OP_BFV_ENCRYPT, 0, 1)
    table("hegpu_bfv_encrypt", "bfv", dict(rng=rng, pk=x, plain=x2, ct=y, ws=ws, ws_bytes=benc, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"ws_bytes": benc - 1}, SMALL),
    ])
    table("hegpu_ckks_decrypt", "ckks", dict(ct=x, sk=x2, depth=0, plain=y, stream=None), [({"ctx": "bfv"}, SCHEME), ({"depth": Q}, DEPTH)])
    bdec = need("bfv", hg.OP_BFV_DECRYPT, 0, 1)
    table("hegpu_bfv_decrypt", "bfv", dict(ct=x, sk=x2, plain=y, ws=ws, ws_bytes=bdec, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"ws_bytes": bdec - 1}, SMALL),
    ])
    table("hegpu_bfv_encode", "bfv", dict(message=x, message_size=N, plain=y, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"message_size": N + 1}, (INV, "Message size can not be higher than the slot count.")),
    ])
    bdcd = need("bfv", hg.OP_BFV_DECODE, 0, 1)
    table("hegpu_bfv_decode", "bfv", dict(plain=x, message=y, ws=ws, ws_bytes=bdcd, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"ws_bytes": bdcd - 1}, SMALL),
    ])
    cenc = need("ckks", hg.OP_CKKS_ENCODE, 0, 1)
    table("hegpu_ckks_encode", "ckks", dict(message=x, message_size=N // 2, scale=2.0 ** 30, plain=y, ws=ws, ws_bytes=cenc, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"message_size": N // 2 + 1}, (INV, "Vector size can not be higher than slot count!")),
        ({"scale": 0.0}, (INV, "Scale out of bounds")),
        ({"ws_bytes": cenc - 1}, SMALL),
        ({"scale": 0.0, "ws_bytes": 0}, (INV, "Scale out of bounds")),
    ])
    table("hegpu_ckks_encode_coeff", "ckks", dict(message=x, message_size=N, scale=2.0 ** 30, plain=y, stream=None), [
        ({"message_size": N + 1}, (INV, "Vector size can not be higher than polynomial degree!")),
    ])
    cdec = need("ckks", hg.OP_CKKS_DECODE, 0, 1)
    table("hegpu_ckks_decode", "ckks", dict(plain=x, depth=0, scale=2.0 ** 30, message=y, ws=ws, ws_bytes=cdec, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"depth": Q}, DEPTH),
        ({"scale": 0.0}, (INV, "scale must be positive")),
        ({"ws_bytes": cdec - 1}, SMALL),
    ])
    table("hegpu_bfv_noise_rns", "bfv", dict(ct=x, sk=x2, out=y, stream=None), [({"ctx": "ckks"}, SCHEME)])
    bmp = need("bfv", hg.OP_BFV_MULTIPLY_PLAIN, 0, 1)
    table("hegpu_bfv_multiply_plain", "bfv", dict(ct=x, plain=x2, out=y, ws=ws, ws_bytes=bmp, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"ws_bytes": bmp - 1}, SMALL),
    ])
    table("hegpu_bfv_plain_addsub", "bfv", dict(ct=x, plain=x2, out=y, sub=0, stream=None), [({"ctx": "ckks"}, SCHEME)])
    table("hegpu_bfv_plain_to_ntt", "bfv", dict(plain=x, out=y, stream=None), [({"ctx": "ckks"}, SCHEME)])

    # ---- ciphertext (x) constant
    table("hegpu_cipherplain_multiplication", "ckks", dict(ct=x, plain=x2, out=y, limbs=Q, stream=None), [({"limbs": 0}, (INV, "bad limb count"))])
    shape = (INV, "bad ciphertext shape")
    table("hegpu_ckks_constant_op", "ckks", dict(op=0, ct=x, value=1.0, out=y, limbs=Q, parts=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"op": 3}, (INV, "unknown constant operation")),
        ({"limbs": 0}, shape),
        ({"parts": 1}, shape),
        ({"value": float("nan")}, (INV, "constant out of range")),
        ({"value": 3.4e38}, (INV, "constant out of range")),
        ({"op": 3, "limbs": 0}, (INV, "unknown constant operation")),
        ({"parts": 1, "value": float("nan")}, shape),
    ])
    table("hegpu_ckks_gaussian_integer_op", "ckks", dict(op=0, ct=x, re=1.0, im=1.0, out=y, limbs=Q, parts=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"op": 2}, (INV, "unknown constant operation")),
        ({"parts": 4}, shape),
        ({"im": float("inf")}, (INV, "constant is not a finite number")),
    ])
    table("hegpu_ckks_mult_i", "ckks", dict(ct=x, out=y, limbs=Q, parts=2, divide=0, stream=None), [({"ctx": "bfv"}, SCHEME), ({"limbs": 0}, shape)])
    table("hegpu_negacyclic_shift", "ckks", dict(src=x, out=y, shift=1, limbs=Q, parts=2, stream=None), [
        ({"out": x}, (INV, "negacyclic shift: out must not alias in")),
        ({"limbs": 0}, shape),
        ({"parts": 0}, shape),
        ({"shift": -1}, (INV, "shift must be in [0, 2N)")),
        ({"out": x, "limbs": 0}, (INV, "negacyclic shift: out must not alias in")),
    ])

    # ---- multiparty keys, decryption and refresh
    mpc = need("ckks", hg.OP_MPC_KEY_SHARE, 0, 1)
    private = (INV, "crs and rng must be different generators: the party's errors are private")
    table("hegpu_mpc_public_key_share", "ckks", dict(crs=crs, rng=rng, sk=x, share=y, ws=ws, ws_bytes=mpc, stream=None), [
        ({"ws_bytes": mpc - 1}, SMALL),
        ({"crs": rng}, private),
        ({"ws_bytes": 0, "crs": rng}, SMALL),
    ])
    table("hegpu_mpc_relin_key_share_round1", "ckks", dict(crs=crs, rng=rng, sk=x, u_out=y2, share=y, ws=ws, ws_bytes=mpc, stream=None), [
        ({"ws_bytes": mpc - 1}, SMALL),
        ({"crs": rng}, private),
    ])
    table("hegpu_mpc_relin_key_share_round2", "ckks", dict(rng=rng, sk=x, u=x2, round1_sum=k, share=y, ws=ws, ws_bytes=mpc, stream=None), [
        ({"ws_bytes": mpc - 1}, SMALL),
        ({"share": k}, (INV, "the share must not overwrite the round-1 sum")),
    ])
    table("hegpu_mpc_galois_key_share", "ckks", dict(crs=crs, rng=rng, sk=x, galois_elt=5, share=y, ws=ws, ws_bytes=mpc, stream=None), [
        ({"ws_bytes": mpc - 1}, SMALL),
        ({"crs": rng}, private),
        ({"galois_elt": 6}, (INV, "galois element must be odd and below 2N")),
        ({"crs": rng, "galois_elt": 6}, private),
    ])
    shares2 = (ctypes.c_void_p * 2)(x, x2)
    with_out = (ctypes.c_void_p * 2)(x, y)
    table("hegpu_mpc_accumulate", "ckks", dict(shares=shares2, k=2, layout=hg.MPC_PUBLIC_KEY, out=y, stream=None), [
        ({"layout": 3}, (INV, "unknown share layout")),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"shares": with_out}, (INV, "the result must not be one of the shares")),
        ({"layout": 3, "k": 0}, (INV, "unknown share layout")),
    ])
    table("hegpu_mpc_relin_key_finish", "ckks", dict(shares=shares2, k=2, round1_sum=k, rk=y, stream=None), [
        ({"rk": k}, (INV, "the key must not overwrite the round-1 sum")),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"shares": with_out}, (INV, "the result must not be one of the shares")),
    ])
    table("hegpu_mpc_ckks_decrypt_share", "ckks", dict(rng=rng, ct=x, cs=S, sk=x2, depth=0, share=y, batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"batch": 0, "depth": Q}, NOOP),
    ])
    table("hegpu_mpc_ckks_decrypt_merge", "ckks", dict(ct=x, cs=S, shares=shares2, k=2, depth=0, plain=y, batch=2, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"shares": with_out}, (INV, "the result must not be one of the shares")),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"depth": Q}, DEPTH),
        ({"k": 0, "batch": 0}, (INV, "at least one share is needed")),  # the shares are looked at before the batch
    ])
    table("hegpu_mpc_bfv_decrypt_share", "bfv", dict(rng=rng, ct=x, cs=S, sk=x2, share=y, batch=2, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
    ])
    bmerge = need("bfv", hg.OP_MPC_BFV_DECRYPT_MERGE)
    table("hegpu_mpc_bfv_decrypt_merge", "bfv", dict(ct=x, cs=S, shares=shares2, k=2, plain=y, batch=2, ws=ws, ws_bytes=bmerge, stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": bmerge - 1}, SMALL),
    ])
    mask = (INV, "crs and rng must be different generators: the party's mask and errors are private")
    rshare = e.ctx["ckks"].workspace_bytes(hg.OP_MPC_REFRESH_SHARE, 0, 2)
    table("hegpu_mpc_ckks_refresh_share", "ckks", dict(crs=crs, rng=rng, ct=x, cs=S, sk=x2, depth=0, mask_bits=20, share=y, batch=2, ws=ws,
                                                       ws_bytes=max(rshare, 8), stream=None), [
        ({"crs": rng}, mask),
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"depth": Q}, DEPTH),
        ({"batch": 0}, NOOP),
        ({"mask_bits": 0}, (INV, "mask_bits must be in [1, 126] with 2^mask_bits below half the level's modulus")),
        ({"mask_bits": 99}, (INV, "mask_bits must be in [1, 126] with 2^mask_bits below half the level's modulus")),
        ({"crs": rng, "ctx": "bfv"}, mask),
        ({"batch": -1, "depth": Q}, NEG),
        ({"batch": 0, "depth": Q}, DEPTH),  # here the depth is looked at before the empty batch leaves
        ({"batch": 0, "mask_bits": 0}, NOOP),
    ] + ([({"ws_bytes": rshare - 1}, SMALL)] if rshare else []))
    rmerge = need("ckks", hg.OP_MPC_REFRESH_MERGE)
    sw = (Q + Q) * N  # a share of the refresh at depth 0
    rshares = (ctypes.c_void_p * 2)(x2, k)
    table("hegpu_mpc_ckks_refresh_merge", "ckks", dict(crs=crs, ct=x, cs=S, shares=rshares, k=2, depth=0, out=y, so=S, batch=2, ws=ws,
                                                       ws_bytes=rmerge, stream=None), [
        ({"ctx": "bfv"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"depth": Q}, DEPTH),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": rmerge - 1}, SMALL),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"shares": (ctypes.c_void_p * 2)(x2, y)}, (INV, "the result must not be one of the shares")),
        ({"so": W - 1}, (INV, "the items of a batch overlap: stride below the size of an item")),
        ({"cs": W - 1}, (INV, "the items of a batch overlap: stride below the size of an item")),
        ({"out": _p(X, W - 1)}, (INV, "the result overlaps the input ciphertexts")),
        ({"out": _p(X2, sw - 1), "batch": 1}, (INV, "the result overlaps a share")),
        ({"batch": 0, "depth": Q}, DEPTH),
        ({"batch": 0, "ws_bytes": 0, "k": 0}, NOOP),
        ({"ws_bytes": 0, "k": 0}, SMALL),
    ])
    bshare = e.ctx["bfv"].workspace_bytes(hg.OP_MPC_REFRESH_SHARE, 0, 2)
    table("hegpu_mpc_bfv_refresh_share", "bfv", dict(crs=crs, rng=rng, ct=x, cs=S, sk=x2, share=y, batch=2, ws=ws, ws_bytes=max(bshare, 8),
                                                     stream=None), [
        ({"crs": rng}, mask),
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
    ])
    brm = need("bfv", hg.OP_MPC_REFRESH_MERGE)
    table("hegpu_mpc_bfv_refresh_merge", "bfv", dict(crs=crs, ct=x, cs=S, shares=rshares, k=2, out=y, so=S, batch=2, ws=ws, ws_bytes=brm,
                                                     stream=None), [
        ({"ctx": "ckks"}, SCHEME),
        ({"batch": -1}, NEG),
        ({"batch": 0}, NOOP),
        ({"ws_bytes": brm - 1}, SMALL),
        ({"k": 0}, (INV, "at least one share is needed")),
        ({"so": W - 1}, (INV, "the items of a batch overlap: stride below the size of an item")),
        ({"out": _p(X, W - 1)}, (INV, "the result overlaps the input ciphertexts")),
        ({"out": _p(X2, W - 1), "batch": 1}, (INV, "the result overlaps a share")),
    ])
    return rows


def test_every_refusal_and_no_op_leaves_the_buffers_alone(env):
    lib = _lib.load()
    rows = _rows(env)
    assert len(rows) > 300
    buffers = (env.X, env.X2, env.Y, env.Y2, env.K, env.WS)
    for ctx, entry, args, (code, text), label in rows:
        rc = getattr(lib, entry)(env.ctx[ctx]._h, *args)
        got = lib.hegpu_last_error().decode() if rc else ""
        print(ctx, label, "->", rc, got)
        assert rc == code, (ctx, label, rc, got)
        if code:
            assert got == text, (ctx, label, got)
    torch.cuda.synchronize()
    for t in buffers:
        assert bool((t == SENT).all()), "a refused or empty call wrote to a buffer"
