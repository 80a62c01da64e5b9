"""CPU: the logic-gate entries of include/hegpu.h are exported by libhegpu.so with the declared argument counts, the two
workspace rows are sized from the rows of the sequence, and every refusal comes before the context is uploaded: on a host-only
context it is HEGPU_E_INVALID with a message, not HEGPU_E_NODEVICE."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"hegpu_ckks_gate_combine": 18, "hegpu_bfv_gate_combine": 13, "hegpu_ckks_logic_gate": 16, "hegpu_bfv_logic_gate": 14}
GATES = ["AND", "OR", "XOR", "NAND", "NOR", "XNOR", "NOT"]
N = 4096


def test_symbols_and_argument_counts(hg):
    from heongpu_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hegpu.h")).read(), flags=re.S)
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name, argc in ENTRIES.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, f"{name} is not declared in hegpu.h"
        assert len(m.group(1).split(",")) == argc, (name, m.group(1))
        assert len(bound[name][2]) == argc, (name, "ctypes signature")


def test_gate_enum_and_workspace_ops(hg):
    header = open(os.path.join(ROOT, "include", "hegpu.h")).read()
    for i, g in enumerate(GATES):
        assert re.search(r"\bHEGPU_LOGIC_%s = %d\b" % (g, i), header), g
        assert getattr(hg, "LOGIC_" + g) == i
    assert "HEGPU_OP_CKKS_LOGIC_GATE = 22" in header and "HEGPU_OP_BFV_LOGIC_GATE = 23" in header
    assert (hg.OP_CKKS_LOGIC_GATE, hg.OP_BFV_LOGIC_GATE) == (22, 23)
    # the TFHE gate numbering stays as it is
    assert (hg.GATE_NAND, hg.GATE_AND, hg.GATE_NOT) == (0, 1, 7)


def test_workspace_rows(hg):
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [40, 30, 30], [40], sec=hg.SEC_NONE)
    for depth, batch in ((0, 1), (1, 2), (0, 3)):
        l = 3 - depth
        want = 3 * l * N * 8 * batch + max(c.workspace_bytes(hg.OP_CKKS_RELIN, depth, batch),
                                           c.workspace_bytes(hg.OP_CKKS_RESCALE, depth, batch))
        assert c.workspace_bytes(hg.OP_CKKS_LOGIC_GATE, depth, batch) == want
    b = hg.Context.from_bit_sizes(hg.BFV, N, [36, 36, 36], [37], plain_modulus=65537, sec=hg.SEC_NONE)
    for batch in (1, 2):
        want = 3 * 3 * N * 8 * batch + max(b.workspace_bytes(op, 0, batch)
                                           for op in (hg.OP_BFV_MULTIPLY, hg.OP_BFV_RELIN, hg.OP_BFV_MULTIPLY_PLAIN))
        assert b.workspace_bytes(hg.OP_BFV_LOGIC_GATE, 0, batch) == want
    # the existing rows are untouched
    assert c.workspace_bytes(hg.OP_CKKS_RELIN, 0, 1) == (3 * 4 + 2 * 4) * N * 8
    assert c.workspace_bytes(24, 0, 1) == 0


def _refused(hg, c, rc, text):
    assert rc == hg.E_INVALID, rc
    assert c._lib.hegpu_last_error().decode() == text


def test_refusals_need_no_device(hg):
    """fake, well-separated addresses: nothing is dereferenced, because every one of these is refused before the upload"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_logic.py checks the refusals there, with the outputs watched")
    c = hg.Context.from_bit_sizes(hg.CKKS, N, [40, 30, 30], [40], sec=hg.SEC_NONE)
    bfv = hg.Context.from_bit_sizes(hg.BFV, N, [36, 36, 36], [37], plain_modulus=65537, sec=hg.SEC_NONE)
    lib = c._lib
    A, B, P, OUT, WS, KEY = (0x10000000 * k for k in range(1, 7))
    w2, w3 = 2 * 2 * N, 2 * 3 * N
    s = 2.0 ** 30
    ok = dict(gate=hg.LOGIC_XOR, a=A, a_stride=w3, a_limbs=3, b=B, b_kind=hg.GATE_B_CIPHER, b_stride=w3, b_limbs=3, p=P,
              p_stride=w2, p_limbs=2, scale_one=s, out=OUT, out_stride=w2, limbs=2, batch=1, stream=None)

    def combine(ctx=c, **change):
        a = dict(ok, **change)
        return lib.hegpu_ckks_gate_combine(ctx._h, *a.values())

    # the baseline is refused by nothing but the missing device
    assert combine() == hg.E_NODEVICE
    _refused(hg, c, combine(gate=7), "hegpu_ckks_gate_combine: unknown gate")
    _refused(hg, c, combine(gate=-1), "hegpu_ckks_gate_combine: unknown gate")
    _refused(hg, c, combine(a_limbs=1), "hegpu_ckks_gate_combine: an operand has fewer limbs than the result")
    _refused(hg, c, combine(b_limbs=1), "hegpu_ckks_gate_combine: an operand has fewer limbs than the result")
    _refused(hg, c, combine(p_limbs=1), "hegpu_ckks_gate_combine: an operand has fewer limbs than the result")
    _refused(hg, c, combine(limbs=0), "hegpu_ckks_gate_combine: bad limb count")
    _refused(hg, c, combine(a_limbs=4), "hegpu_ckks_gate_combine: an operand has fewer limbs than the result")
    _refused(hg, c, combine(batch=32768), "hegpu_ckks_gate_combine: at most 32767 items per call")
    _refused(hg, c, combine(batch=-1), "hegpu_ckks_gate_combine: batch must not be negative")
    _refused(hg, c, combine(out=A), "hegpu_ckks_gate_combine: out is an operand itself (equal strides and limb counts) or does not overlap it")                          # a has 3 limbs, out 2: no in-place form
    _refused(hg, c, combine(out=B + 8), "hegpu_ckks_gate_combine: out is an operand itself (equal strides and limb counts) or does not overlap it")
    _refused(hg, c, combine(out=P), "hegpu_ckks_gate_combine: out must not overlap the product")
    _refused(hg, c, combine(scale_one=0.0), "hegpu_ckks_gate_combine: the scale of the constant one is positive and below 3.4e38")
    _refused(hg, c, combine(scale_one=float("nan")), "hegpu_ckks_gate_combine: the scale of the constant one is positive and below 3.4e38")
    _refused(hg, c, combine(gate=hg.LOGIC_NOT), "hegpu_ckks_gate_combine: NOT takes no second operand and no product, every other gate takes both")              # NOT with a second operand
    _refused(hg, c, combine(b_kind=hg.GATE_B_NONE), "hegpu_ckks_gate_combine: NOT takes no second operand and no product, every other gate takes both")
    _refused(hg, c, combine(p=None), "hegpu_ckks_gate_combine: null argument")
    _refused(hg, c, combine(ctx=bfv), "context scheme mismatch")                        # wrong scheme
    assert combine(batch=0) == 0
    # a CKKS NOT in place is allowed: refused by nothing but the missing device
    assert combine(gate=hg.LOGIC_NOT, b=None, b_kind=hg.GATE_B_NONE, p=None, out=A, out_stride=w3, limbs=3) == hg.E_NODEVICE

    wq = 2 * 3 * N
    assert lib.hegpu_bfv_gate_combine(bfv._h, hg.LOGIC_OR, A, wq, B, hg.GATE_B_CIPHER, wq, P, wq, A, wq, 2, None) == hg.E_NODEVICE
    _refused(hg, bfv, lib.hegpu_bfv_gate_combine(bfv._h, hg.LOGIC_OR, A, wq, B, hg.GATE_B_CIPHER, wq, P, wq, A + 8, wq, 2, None), "hegpu_bfv_gate_combine: out is an operand itself (equal strides and limb counts) or does not overlap it")
    _refused(hg, bfv, lib.hegpu_bfv_gate_combine(bfv._h, hg.LOGIC_OR, A, wq, B, hg.GATE_B_PLAIN, N, P, wq, B, wq, 2, None), "hegpu_bfv_gate_combine: out is an operand itself (equal strides and limb counts) or does not overlap it")
    _refused(hg, bfv, lib.hegpu_bfv_gate_combine(c._h, hg.LOGIC_OR, A, wq, B, hg.GATE_B_CIPHER, wq, P, wq, OUT, wq, 2, None), "context scheme mismatch")

    need = c.workspace_bytes(hg.OP_CKKS_LOGIC_GATE, 0, 2)

    def gate(ctx=c, gate=hg.LOGIC_NOR, a=A, b=B, kind=hg.GATE_B_CIPHER, key=KEY, scale=s, out=OUT, depth=0, batch=2, ws=WS,
             ws_bytes=need):
        return lib.hegpu_ckks_logic_gate(ctx._h, gate, a, w3, b, kind, w3, key, scale, out, w2, depth, batch, ws, ws_bytes, None)

    assert gate() == hg.E_NODEVICE
    _refused(hg, c, gate(gate=9), "hegpu_ckks_logic_gate: unknown gate")
    _refused(hg, c, gate(ws_bytes=need - 8), "workspace too small")
    _refused(hg, c, gate(ws=None), "workspace too small")
    _refused(hg, c, gate(key=None), "hegpu_ckks_logic_gate: null argument")
    _refused(hg, c, gate(out=A), "hegpu_ckks_logic_gate: out is an operand itself (equal strides and limb counts) or does not overlap it")
    _refused(hg, c, gate(out=WS), "hegpu_ckks_logic_gate: the workspace must overlap neither out nor an operand")
    _refused(hg, c, gate(depth=2), "hegpu_ckks_logic_gate: no modulus left to rescale the product by")                           # a binary gate on the last level
    _refused(hg, c, gate(depth=3), "invalid depth")
    _refused(hg, c, gate(batch=40000), "hegpu_ckks_logic_gate: at most 32767 items per call")
    _refused(hg, c, gate(ctx=bfv), "context scheme mismatch")
    _refused(hg, c, gate(scale=0.0), "hegpu_ckks_logic_gate: the scale of the constant one is positive and below 3.4e38")
    needb = bfv.workspace_bytes(hg.OP_BFV_LOGIC_GATE, 0, 1)
    assert lib.hegpu_bfv_logic_gate(bfv._h, hg.LOGIC_AND, A, wq, B, hg.GATE_B_CIPHER, wq, KEY, A, wq, 1, WS, needb, None) == hg.E_NODEVICE
    _refused(hg, bfv, lib.hegpu_bfv_logic_gate(bfv._h, hg.LOGIC_AND, A, wq, B, hg.GATE_B_CIPHER, wq, KEY, A, wq, 1, WS, needb - 8, None), "workspace too small")
    _refused(hg, bfv, lib.hegpu_bfv_logic_gate(c._h, hg.LOGIC_AND, A, wq, B, hg.GATE_B_CIPHER, wq, KEY, OUT, wq, 1, WS, needb, None), "context scheme mismatch")
