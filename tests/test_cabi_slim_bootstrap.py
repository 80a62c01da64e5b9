"""The C ABI of the slim, bit and gate refreshes without a device: the symbols, the workspace query and every refusal of
hegpu_ckks_slim_bootstrap and hegpu_ckks_conj_real, which are all decided on the host tables before the context is
uploaded.  Every buffer here is host memory that no call may touch: each call below is refused."""
import numpy as np
import pytest
import torch

import heongpu_amd as hg
from heongpu_amd import _lib

N = 4096
DELTA = 2.0 ** 40
CHAIN = ([50, 40, 40, 40, 40, 40] + [50] * 8 + [50] + [50] * 3, [60])
SENT = 0x5555555555555555


@pytest.fixture(scope="module")
def setup():
    c = hg.Context.from_bit_sizes(hg.CKKS, N, *CHAIN, sec=hg.SEC_NONE)
    primes = [int(x) for x in c.table("modulus")]
    plan = hg.slim_bootstrap_plan(primes[:c.Q_size], DELTA, c.Q_size - 1, "and")
    key = torch.zeros(8, dtype=torch.int64)  # stands for a device key: never read
    cts, stc, elts = c.slim_bootstrap_factors(plan, lambda e: key, lambda values, scale, limbs: torch.zeros(limbs * N, dtype=torch.int64))
    return c, primes, plan, cts, stc, key, elts


def test_symbols_and_the_workspace(setup):
    c, primes, plan, cts, stc, key, elts = setup
    lib = _lib.load()
    bound = {s[0] for s in _lib.SIGNATURES}
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "hegpu.h")).read()
    for name in ("hegpu_eval_trig_plan_size", "hegpu_eval_trig_plan_fill", "hegpu_slim_bootstrap_plan_fill", "hegpu_ckks_conj_real",
                 "hegpu_ckks_slim_bootstrap_workspace_bytes", "hegpu_ckks_slim_bootstrap"):
        assert hasattr(lib, name) and name in bound and name + "(" in header
    # no row of the HEGPU_OP_* table is taken: the rows the existing tests hold at zero stay zero, 28 too
    for row in (24, 27, 28):
        assert c.workspace_bytes(row, 0, 1) == 0
    assert "= 27" not in header and "= 28" not in header
    one = c.slim_bootstrap_workspace_bytes(plan, cts, stc, 1)
    raised, real = 2 * (plan.cts_level + 1) * N * 8, 2 * (plan.eval_level + 1) * N * 8
    assert one > c.workspace_bytes(hg.OP_CKKS_MOD_RAISE, 0, 1) + raised + real
    assert c.slim_bootstrap_workspace_bytes(plan, cts, stc, 2) > one
    assert c.slim_bootstrap_workspace_bytes(plan, cts[:2], stc, 1) == 0 and c.slim_bootstrap_workspace_bytes(plan, cts, stc, 0) == 0
    # the stages of the special FFT are the regular refresh's: the same Galois elements serve both
    regular = hg.bootstrap_plan(primes[:c.Q_size], DELTA, c.Q_size - 1, K=12)
    _, _, regular_elts = c.bootstrap_factors(regular, lambda e: key, lambda values, scale, limbs: torch.zeros(limbs * N, dtype=torch.int64))
    assert elts == regular_elts and 2 * N - 1 in elts
    # SlotToCoeff factor g sits at level in_level - g
    assert [f[0].numel() // (N * f[1]) for f in stc] == [4, 3, 2]
    assert [f[0].numel() // (N * f[1]) for f in cts] == [18, 17, 16]


def test_slim_bootstrap_refusals_need_no_device(setup):
    c, primes, plan, cts, stc, key, elts = setup
    Q = c.Q_size
    in_words, room = 2 * (plan.in_level + 1) * N, 2 * plan.trig.out_limbs * N
    ct = torch.full((in_words,), SENT, dtype=torch.int64)
    ct2 = torch.full((in_words,), SENT, dtype=torch.int64)
    out = torch.full((room,), SENT, dtype=torch.int64)
    ws = torch.full((c.slim_bootstrap_workspace_bytes(plan, cts, stc, 1) // 8,), SENT, dtype=torch.int64)

    def refused(text, **kw):
        args = dict(ct=ct, ct2=ct2, out=out, plan=plan, cts=cts, stc=stc, conj=key, relin=key, batch=1, ws=ws)
        args.update(kw)
        with pytest.raises(hg.HEError) as e:
            c.ckks_slim_bootstrap(args["ct"], in_words, args["out"], room, args["plan"], args["cts"], args["stc"], args["conj"],
                                  args["relin"], args["batch"], args["ws"], ct2=args["ct2"], cs2=in_words, stream=0)
        assert e.value.code == hg.E_INVALID, e.value
        assert str(e.value) == f"[{hg.E_INVALID}] {text}"
        for t in (ct, ct2, out, ws):
            assert bool((t == SENT).all())

    refused("slim_bootstrap: batch must be at least 1", batch=0)
    refused("slim_bootstrap: batch must be at least 1", batch=-1)
    refused("slim_bootstrap: at most 16383 items per call", batch=16384)
    refused("workspace too small", ws=ws[:ws.numel() - 1])
    refused("slim_bootstrap: null argument", ws=None)
    refused("slim_bootstrap: null argument", ct=None)
    refused("slim_bootstrap: null argument", out=None)
    refused("slim_bootstrap: null argument", conj=None)
    refused("slim_bootstrap: null argument", relin=None)
    refused("slim_bootstrap: as many factors as the plan has pieces", cts=cts[:2])
    refused("slim_bootstrap: as many factors as the plan has pieces", stc=stc + stc[:1])
    refused("slim_bootstrap: the raise goes to a level the context has",
            plan=hg.slim_bootstrap_plan(primes[:Q] + [primes[Q - 1]], DELTA, Q, "and"))
    not_the_plan = "slim_bootstrap: the polynomial plan is not the one of the bootstrap plan"
    other = hg.eval_trig_plan(12, 30, 3, plan.phase, plan.amplitude, plan.offset, plan.eval_level, plan.eval_in_scale, 2.0 ** 49, primes[:Q])
    refused(not_the_plan, plan=hg.SlimBootstrapPlan(plan.c, other))
    shorter = hg.eval_trig_plan(12, 30, 2, plan.phase, plan.amplitude, plan.offset, plan.eval_level, plan.eval_in_scale,
                                plan.eval_target_scale, primes[:Q])
    refused(not_the_plan, plan=hg.SlimBootstrapPlan(plan.c, shorter))
    two_pieces = hg.slim_bootstrap_plan(primes[:Q], DELTA, Q - 1, "and", stc_pieces=2)
    refused("slim_bootstrap: as many factors as the plan has pieces", plan=two_pieces)
    # an earlier refusal wins: the factor count before the caller's pointers
    refused("slim_bootstrap: as many factors as the plan has pieces", cts=cts[:2], ct=None)
    refused("slim_bootstrap: null argument", ct=None, ws=ws[:1])
    both = torch.full((in_words + room,), SENT, dtype=torch.int64)
    overlap = "slim_bootstrap: out must overlap neither ct nor ct2"
    refused(overlap, ct=both[:in_words], out=both[in_words - 1:in_words - 1 + room])
    refused(overlap, ct2=both[:in_words], out=both[in_words - 1:in_words - 1 + room])
    ws_overlap = "slim_bootstrap: the workspace must overlap neither out nor ct nor ct2"
    refused(ws_overlap, out=ws[:room])
    refused(ws_overlap, ct=ws[:in_words])
    refused(ws_overlap, ct2=ws[ws.numel() - in_words:])
    assert bool((both == SENT).all())
    bfv = hg.Context.from_bit_sizes(hg.BFV, N, [40, 40], [40], plain_modulus=65537, sec=hg.SEC_NONE)
    with pytest.raises(hg.HEError) as e:
        bfv.ckks_slim_bootstrap(ct, in_words, out, room, plan, cts, stc, key, key, 1, ws, stream=0)
    assert e.value.code == hg.E_INVALID
    assert np.all(out.numpy().view(np.uint64) == SENT)


def test_conj_real_refusals_need_no_device(setup):
    c = setup[0]
    Q = c.Q_size
    depth = Q - 3
    words = 2 * 3 * N
    x = torch.full((2 * words,), SENT, dtype=torch.int64)
    xc = torch.full((2 * words,), SENT, dtype=torch.int64)
    out = torch.full((2 * words,), SENT, dtype=torch.int64)

    def refused(text, **kw):
        a = dict(x=x, xs=words, xc=xc, xcs=words, out=out, so=words, depth=depth, out_depth=depth, batch=2)
        a.update(kw)
        with pytest.raises(hg.HEError) as e:
            c.ckks_conj_real(a["x"], a["xs"], a["xc"], a["xcs"], a["out"], a["so"], a["depth"], a["out_depth"], a["batch"], stream=0)
        assert e.value.code == hg.E_INVALID, e.value
        assert str(e.value) == f"[{hg.E_INVALID}] {text}"
        for t in (x, xc, out):
            assert bool((t == SENT).all())

    refused("conj_real: batch must be at least 1", batch=0)
    refused("conj_real: at most 32767 items per call", batch=32768)
    refused("conj_real: depth <= out_depth < Q", out_depth=depth - 1)
    refused("conj_real: depth <= out_depth < Q", out_depth=Q)
    refused("conj_real: depth <= out_depth < Q", depth=-1)
    refused("conj_real: null argument", x=None)
    refused("conj_real: null argument", xc=None)
    refused("conj_real: null argument", out=None)
    refused("conj_real: out must not overlap xc", out=xc)
    refused("conj_real: out must not overlap xc", out=xc[words - 1:], batch=1)
    in_place = "conj_real: out is x itself (equal strides and depths) or does not overlap it"
    refused(in_place, out=x[1:], batch=1)
    refused(in_place, out=x, out_depth=depth + 1)         # fewer limbs: the parts move
    refused(in_place, out=x, so=words + N, xs=words, batch=1)
    bfv = hg.Context.from_bit_sizes(hg.BFV, N, [40, 40], [40], plain_modulus=65537, sec=hg.SEC_NONE)
    with pytest.raises(hg.HEError) as e:
        bfv.ckks_conj_real(x, words, xc, words, out, words, 0, 0, 1, stream=0)
    assert e.value.code == hg.E_INVALID and "context scheme mismatch" in str(e.value)
