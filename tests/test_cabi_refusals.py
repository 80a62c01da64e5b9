"""CPU: what the entries that check their arguments BEFORE the context is uploaded refuse, as a table of
(entry, arguments) -> (return code, exact hegpu_last_error() text), in each entry's own order of checks.  Every row is a
refusal or an empty-batch no-op: nothing is uploaded and no address is dereferenced, so the device pointers are made-up,
well-separated addresses.  The later refusals of hegpu_ckks_bootstrap need a chain a refresh fits in: tests/test_cabi_bootstrap.py
holds those."""
import ctypes

import pytest

import heongpu_amd as hg
from heongpu_amd import _lib

N = 4096
Q = 3
INV = hg.E_INVALID
A, B, P, OUT, WS, KEY = (0x10000000 * k for k in range(1, 7))
W1, W2, W3 = 2 * 1 * N, 2 * 2 * N, 2 * 3 * N
S = 2.0 ** 30


@pytest.fixture(scope="module")
def ctxs():
    ckks = hg.Context.from_bit_sizes(hg.CKKS, N, [40, 30, 30], [40], sec=hg.SEC_NONE)
    bfv = hg.Context.from_bit_sizes(hg.BFV, N, [40, 30, 30], [40], plain_modulus=65537, sec=hg.SEC_NONE)
    return {"ckks": ckks, "bfv": bfv, None: None}


def _rows(ctxs):
    ckks = ctxs["ckks"]
    raise_need = ckks.workspace_bytes(hg.OP_CKKS_MOD_RAISE, 0, 2)
    gate_need = ckks.workspace_bytes(hg.OP_CKKS_LOGIC_GATE, 0, 2)
    bgate_need = ctxs["bfv"].workspace_bytes(hg.OP_BFV_LOGIC_GATE, 0, 2)
    plan, steps = _lib.BootstrapPlan(), (_lib.PolyStep * 1)()
    factor = (_lib.LinearFactor * 1)()
    rows, bases = [], {}

    def table(entry, ok, cases):
        bases[entry] = ok
        for change, want in cases:
            rows.append((entry, dict(ok, **change), want, (entry, change)))

    # ---- the two ordered transforms: the order table is asked for before anything else, the context included
    order_ok = dict(ctx="ckks", table_set=hg.TABLES_QP, inout=A, inverse=0, mod_offset=0, batch=1, mod_count=1, order=None, stream=None)
    table("hegpu_GPU_NTT_Modulus_Ordered_Inplace", order_ok, [
        ({}, (INV, "modulus order table is required")),
        ({"ctx": None}, (INV, "modulus order table is required")),
    ])
    table("hegpu_GPU_NTT_Poly_Ordered_Inplace", order_ok, [
        ({}, (INV, "polynomial order table is required")),
        ({"ctx": None}, (INV, "polynomial order table is required")),
    ])

    # ---- hegpu_mod_raise
    ok = dict(ctx="ckks", src=A, in_stride=2 * N, out=OUT, out_stride=W3, limbs=3, parts=2, batch=2, stream=None)
    table("hegpu_mod_raise", ok, [
        ({"ctx": None}, (INV, "null context")),
        ({"src": None}, (INV, "mod_raise: null argument")),
        ({"out": None}, (INV, "mod_raise: null argument")),
        ({"batch": 0}, (INV, "mod_raise: 1 to 65535 items per call")),
        ({"batch": -1}, (INV, "mod_raise: 1 to 65535 items per call")),
        ({"batch": 65536}, (INV, "mod_raise: 1 to 65535 items per call")),
        ({"parts": 0}, (INV, "mod_raise: parts is 1, 2 or 3")),
        ({"parts": 4}, (INV, "mod_raise: parts is 1, 2 or 3")),
        ({"limbs": 0}, (INV, "mod_raise: 1 <= limbs <= Q")),
        ({"limbs": Q + 1}, (INV, "mod_raise: 1 <= limbs <= Q")),
        ({"out": A + 8 * (2 * N - 1)}, (INV, "mod_raise: out must not overlap in")),
        ({"out": A + 8 * 2 * N, "in_stride": 2 * N + W3, "out_stride": 2 * N + W3, "batch": 65536},
         (INV, "mod_raise: 1 to 65535 items per call")),
        # an earlier refusal wins
        ({"src": None, "batch": 0, "parts": 0}, (INV, "mod_raise: null argument")),
        ({"batch": 0, "parts": 0, "limbs": 0}, (INV, "mod_raise: 1 to 65535 items per call")),
        ({"parts": 0, "limbs": 0, "out": A}, (INV, "mod_raise: parts is 1, 2 or 3")),
    ])

    # ---- hegpu_ckks_mod_raise
    ok = dict(ctx="ckks", ct=A, cs=W1, out=OUT, so=W3, out_depth=0, batch=2, ws=WS, ws_bytes=raise_need, stream=None)
    table("hegpu_ckks_mod_raise", ok, [
        ({"ctx": None}, (INV, "null context")),
        ({"ctx": "bfv"}, (INV, "context scheme mismatch")),
        ({"ct": None}, (INV, "ckks_mod_raise: null argument")),
        ({"out": None}, (INV, "ckks_mod_raise: null argument")),
        ({"ws": None}, (INV, "ckks_mod_raise: null argument")),
        ({"batch": 0}, (INV, "ckks_mod_raise: batch must be at least 1")),
        ({"batch": -1}, (INV, "ckks_mod_raise: batch must be at least 1")),
        ({"out_depth": -1}, (INV, "ckks_mod_raise: 0 <= out_depth < Q")),
        ({"out_depth": Q}, (INV, "ckks_mod_raise: 0 <= out_depth < Q")),
        ({"ws_bytes": raise_need - 1}, (INV, "workspace too small")),
        ({"out": A + 8 * (W1 - 1)}, (INV, "ckks_mod_raise: out must not overlap ct")),
        ({"ws": OUT + 8 * (2 * W3 - 1)}, (INV, "ckks_mod_raise: the workspace must overlap neither out nor ct")),
        ({"ws": A - raise_need + 8}, (INV, "ckks_mod_raise: the workspace must overlap neither out nor ct")),
        # an earlier refusal wins
        ({"ctx": "bfv", "ct": None, "batch": 0}, (INV, "context scheme mismatch")),
        ({"ws": None, "batch": 0, "out_depth": Q}, (INV, "ckks_mod_raise: null argument")),
        ({"batch": 0, "out_depth": Q, "ws_bytes": 0}, (INV, "ckks_mod_raise: batch must be at least 1")),
        ({"ws_bytes": 0, "out": A}, (INV, "workspace too small")),
    ])

    # ---- hegpu_ckks_bootstrap, as far as a three-limb chain reaches (no refresh fits in it: the plan is refused)
    ok = dict(ctx="ckks", ct=A, cs=W1, out=OUT, so=W3, plan=ctypes.pointer(plan), eval_mod=steps, n_steps=1, cts=factor,
              cts_count=1, stc=factor, stc_count=1, conj_key=KEY, relin_key=KEY, d2s=None, s2d=None, batch=1, ws=WS,
              ws_bytes=1 << 20, stream=None)
    table("hegpu_ckks_bootstrap", ok, [
        ({"ctx": None}, (INV, "null context")),
        ({"ctx": "bfv"}, (INV, "context scheme mismatch")),
        ({"plan": None}, (INV, "bootstrap: null argument")),
        ({"eval_mod": None}, (INV, "bootstrap: null argument")),
        ({"cts": None}, (INV, "bootstrap: null argument")),
        ({"stc": None}, (INV, "bootstrap: null argument")),
        ({"batch": 0}, (INV, "bootstrap: batch must be at least 1")),
        ({"batch": -1}, (INV, "bootstrap: batch must be at least 1")),
        ({"batch": 16384}, (INV, "bootstrap: at most 16383 items per call")),
        ({}, (INV, "bootstrap: a piece count outside [1, 5]")),
        # an earlier refusal wins
        ({"ctx": "bfv", "plan": None, "batch": 0}, (INV, "context scheme mismatch")),
        ({"stc": None, "batch": 0}, (INV, "bootstrap: null argument")),
        ({"batch": 16384, "ct": None}, (INV, "bootstrap: at most 16383 items per call")),
    ])

    # ---- the one-pass combine
    for scheme, entry in (("ckks", "hegpu_ckks_gate_combine"), ("bfv", "hegpu_bfv_gate_combine")):
        other = "bfv" if scheme == "ckks" else "ckks"
        if scheme == "ckks":
            ok = dict(ctx="ckks", gate=hg.LOGIC_XOR, a=A, a_stride=W3, a_limbs=3, b=B, b_kind=hg.GATE_B_CIPHER, b_stride=W3,
                      b_limbs=3, p=P, p_stride=W2, p_limbs=2, scale_one=S, out=OUT, out_stride=W2, limbs=2, batch=2, stream=None)
        else:
            ok = dict(ctx="bfv", gate=hg.LOGIC_XOR, a=A, a_stride=W3, b=B, b_kind=hg.GATE_B_CIPHER, b_stride=W3, p=P,
                      p_stride=W3, out=OUT, out_stride=W3, batch=2, stream=None)
        own = ok["out_stride"]
        NOT = {"gate": hg.LOGIC_NOT, "b": None, "b_kind": hg.GATE_B_NONE, "p": None}
        cases = [
            ({"ctx": None}, (INV, "null context")),
            ({"ctx": other}, (INV, "context scheme mismatch")),
            ({"gate": 7}, (INV, entry + ": unknown gate")),
            ({"gate": -1}, (INV, entry + ": unknown gate")),
            ({"batch": -1}, (INV, entry + ": batch must not be negative")),
            ({"batch": 32768}, (INV, entry + ": at most 32767 items per call")),
            ({"batch": 0}, (0, None)),
            ({"batch": 0, "a": None, "out": None}, (0, None)),  # the empty batch leaves before the operands are looked at
            ({"gate": hg.LOGIC_NOT}, (INV, entry + ": NOT takes no second operand and no product, every other gate takes both")),
            (dict(NOT, p=P), (INV, entry + ": NOT takes no second operand and no product, every other gate takes both")),
            ({"b_kind": hg.GATE_B_NONE}, (INV, entry + ": NOT takes no second operand and no product, every other gate takes both")),
            ({"b_kind": 3}, (INV, entry + ": NOT takes no second operand and no product, every other gate takes both")),
            ({"a": None}, (INV, entry + ": null argument")),
            ({"out": None}, (INV, entry + ": null argument")),
            ({"b": None}, (INV, entry + ": null argument")),
            ({"p": None}, (INV, entry + ": null argument")),
            (dict(NOT, a=None), (INV, entry + ": null argument")),
        ]
        if scheme == "ckks":
            cases += [
                ({"limbs": 0}, (INV, entry + ": bad limb count")),
                ({"limbs": Q + 1}, (INV, entry + ": bad limb count")),
                ({"a_limbs": 1}, (INV, entry + ": an operand has fewer limbs than the result")),
                ({"a_limbs": Q + 1}, (INV, entry + ": an operand has fewer limbs than the result")),
                ({"b_limbs": 1}, (INV, entry + ": an operand has fewer limbs than the result")),
                ({"p_limbs": 1}, (INV, entry + ": an operand has fewer limbs than the result")),
                ({"scale_one": 0.0}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                ({"scale_one": float("nan")}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                ({"scale_one": 3.4e38}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                ({"out": A}, (INV, entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it")),
                # an earlier refusal wins
                ({"limbs": 0, "a_limbs": 0, "scale_one": 0.0}, (INV, entry + ": bad limb count")),
                ({"a_limbs": 1, "scale_one": 0.0, "out": A}, (INV, entry + ": an operand has fewer limbs than the result")),
                ({"scale_one": 0.0, "out": A}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
            ]
        cases += [
            ({"out": A + 8}, (INV, entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it")),
            ({"out": B + 8}, (INV, entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it")),
            ({"b_kind": hg.GATE_B_PLAIN, "out": B}, (INV, entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it")),
            ({"out": P}, (INV, entry + ": out must not overlap the product")),
            ({"out": P - 8 * (2 * own - 1)}, (INV, entry + ": out must not overlap the product")),
            # an earlier refusal wins
            ({"ctx": other, "gate": 7, "batch": -1}, (INV, "context scheme mismatch")),
            ({"gate": 7, "batch": -1}, (INV, entry + ": unknown gate")),
            ({"gate": 7, "batch": 0}, (INV, entry + ": unknown gate")),
            ({"batch": 32768, "a": None}, (INV, entry + ": at most 32767 items per call")),
            ({"b_kind": 3, "a": None}, (INV, entry + ": NOT takes no second operand and no product, every other gate takes both")),
            ({"out": A + 8, "p": A + 8}, (INV, entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it")),
        ]
        table(entry, ok, cases)

    # ---- the whole gate
    for scheme, entry in (("ckks", "hegpu_ckks_logic_gate"), ("bfv", "hegpu_bfv_logic_gate")):
        other = "bfv" if scheme == "ckks" else "ckks"
        if scheme == "ckks":
            need, so = gate_need, W2
            ok = dict(ctx="ckks", gate=hg.LOGIC_NOR, a=A, a_stride=W3, b=B, b_kind=hg.GATE_B_CIPHER, b_stride=W3, relin_key=KEY,
                      scale_one=S, out=OUT, out_stride=so, depth=0, batch=2, ws=WS, ws_bytes=need, stream=None)
        else:
            need, so = bgate_need, W3
            ok = dict(ctx="bfv", gate=hg.LOGIC_NOR, a=A, a_stride=W3, b=B, b_kind=hg.GATE_B_CIPHER, b_stride=W3, relin_key=KEY,
                      out=OUT, out_stride=so, batch=2, ws=WS, ws_bytes=need, stream=None)
        NOT = {"gate": hg.LOGIC_NOT, "b": None, "b_kind": hg.GATE_B_NONE}
        alias = entry + ": out is an operand itself (equal strides and limb counts) or does not overlap it"
        cases = [
            ({"ctx": None}, (INV, "null context")),
            ({"ctx": other}, (INV, "context scheme mismatch")),
            ({"gate": 7}, (INV, entry + ": unknown gate")),
            ({"batch": -1}, (INV, entry + ": batch must not be negative")),
            ({"batch": 32768}, (INV, entry + ": at most 32767 items per call")),
            ({"batch": 0}, (0, None)),
            ({"batch": 0, "a": None, "ws": None}, (0, None)),  # the empty batch leaves before anything else is looked at
        ]
        if scheme == "ckks":
            cases += [
                ({"depth": -1}, (INV, "invalid depth")),
                ({"depth": Q}, (INV, "invalid depth")),
                ({"batch": 0, "depth": Q}, (0, None)),
            ]
        cases += [
            ({"gate": hg.LOGIC_NOT}, (INV, entry + ": NOT takes no second operand, every other gate a ciphertext or a plaintext")),
            ({"b_kind": hg.GATE_B_NONE}, (INV, entry + ": NOT takes no second operand, every other gate a ciphertext or a plaintext")),
            ({"b_kind": 3}, (INV, entry + ": NOT takes no second operand, every other gate a ciphertext or a plaintext")),
            ({"a": None}, (INV, entry + ": null argument")),
            ({"out": None}, (INV, entry + ": null argument")),
            ({"b": None}, (INV, entry + ": null argument")),
            ({"relin_key": None}, (INV, entry + ": null argument")),
            (dict(NOT, a=None), (INV, entry + ": null argument")),
        ]
        if scheme == "ckks":
            cases += [
                ({"depth": Q - 1}, (INV, entry + ": no modulus left to rescale the product by")),
                ({"scale_one": 0.0}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                ({"scale_one": float("inf")}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                (dict(NOT, scale_one=-1.0), (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
                # an earlier refusal wins
                ({"depth": Q, "b_kind": 3}, (INV, "invalid depth")),
                ({"depth": Q - 1, "scale_one": 0.0, "ws": None}, (INV, entry + ": no modulus left to rescale the product by")),
                ({"scale_one": 0.0, "ws": None}, (INV, entry + ": the scale of the constant one is positive and below 3.4e38")),
            ]
        cases += [
            ({"ws": None}, (INV, "workspace too small")),
            ({"ws_bytes": need - 1}, (INV, "workspace too small")),
            ({"out": A + 8}, (INV, alias)),
            (dict(NOT, out=A + 8, out_stride=W3), (INV, alias)),
            ({"out": B + 8}, (INV, alias)),
            ({"b_kind": hg.GATE_B_PLAIN, "relin_key": None, "out": B}, (INV, alias)),
            ({"ws": OUT + 8 * (2 * so - 1)}, (INV, entry + ": the workspace must overlap neither out nor an operand")),
            ({"ws": A + 8 * (2 * W3 - 1)}, (INV, entry + ": the workspace must overlap neither out nor an operand")),
            ({"ws": B - need + 8}, (INV, entry + ": the workspace must overlap neither out nor an operand")),
            # an earlier refusal wins
            ({"ctx": other, "gate": 7}, (INV, "context scheme mismatch")),
            ({"gate": 7, "batch": 0}, (INV, entry + ": unknown gate")),
            ({"batch": 32768, "b_kind": 3}, (INV, entry + ": at most 32767 items per call")),
            ({"b_kind": 3, "a": None}, (INV, entry + ": NOT takes no second operand, every other gate a ciphertext or a plaintext")),
            ({"a": None, "ws_bytes": 0}, (INV, entry + ": null argument")),
            ({"ws_bytes": 0, "out": A + 8}, (INV, "workspace too small")),
            ({"out": A + 8, "ws": A}, (INV, alias)),
        ]
        table(entry, ok, cases)
    return rows, bases


def _no_device():
    """These tables hand out made-up addresses: with a device present a row that a regression accepted would be launched
    on them.  tests/test_gpu_refusals.py, test_gpu_logic.py and test_gpu_bootstrap.py hold the device side, on real buffers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: the refusals are checked there on real buffers")


def test_every_refusal_and_its_text(ctxs):
    _no_device()
    lib = _lib.load()
    rows, _ = _rows(ctxs)
    assert len(rows) > 150
    for entry, args, (code, text), label in rows:
        ctx = ctxs[args["ctx"]]
        values = [ctx._h if ctx is not None else None] + [v for k, v in args.items() if k != "ctx"]
        rc = getattr(lib, entry)(*values)
        got = lib.hegpu_last_error().decode()
        print(label, "->", rc, got if rc else "")
        assert rc == code, (label, rc, got)
        if code:
            assert got == text, (label, got)


def test_the_unchanged_call_passes_every_check(ctxs):
    """The base row of each table is refused by nothing: without a device it ends in HEGPU_E_NODEVICE, the upload's own
    refusal.  (With a device the made-up addresses would be used: there tests/test_gpu_refusals.py and the operator tests
    hold the accepted calls.)"""
    _no_device()
    lib = _lib.load()
    for entry, args in _rows(ctxs)[1].items():
        if "Ordered" in entry or entry == "hegpu_ckks_bootstrap":
            continue  # their base rows are refusals themselves
        rc = getattr(lib, entry)(*([ctxs[args["ctx"]]._h] + [v for k, v in args.items() if k != "ctx"]))
        assert rc == hg.E_NODEVICE, (entry, rc, lib.hegpu_last_error().decode())
