"""The C ABI of the CKKS refresh without a device: the symbols, the workspace row and every refusal of
hegpu_ckks_bootstrap, which are all decided on the host tables before the context is uploaded.  Every buffer here is host
memory that no call may touch: each call below is refused."""
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
    plan = hg.bootstrap_plan(primes[:c.Q_size], DELTA, c.Q_size - 1, K=12)
    key = torch.zeros(8, dtype=torch.int64)  # stands for a device key: never read
    cts, stc, elts = c.bootstrap_factors(plan, lambda e: key, lambda values, scale, limbs: torch.zeros(limbs * N, dtype=torch.int64))
    return c, primes, plan, cts, stc, key, elts


def test_symbols_and_the_workspace_row(setup):
    c, primes, plan, cts, stc, key, elts = setup
    lib = _lib.load()
    for name in ("hegpu_bootstrap_plan_fill", "hegpu_ckks_bootstrap_workspace_bytes", "hegpu_ckks_bootstrap"):
        assert hasattr(lib, name)
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "hegpu.h")).read()
    assert "HEGPU_OP_CKKS_BOOTSTRAP = 26" in header and hg.OP_CKKS_BOOTSTRAP == 26
    for depth in (0, 5, c.Q_size - 1):
        for batch in (1, 3):
            assert c.workspace_bytes(hg.OP_CKKS_BOOTSTRAP, depth, batch) == 3 * c.workspace_bytes(hg.OP_CKKS_MOD_RAISE, depth, batch) == 6 * N * 8 * batch
    assert c.workspace_bytes(24, 0, 1) == 0 and c.workspace_bytes(27, 0, 1) == 0
    assert c.workspace_bytes(hg.OP_CKKS_BOOTSTRAP, 0, 0) == 0
    # the whole workspace: the head, the raised ciphertext (twice with switch keys), the halves, the sines, a step's workspace
    without, with_keys = c.bootstrap_workspace_bytes(plan, cts, stc, False, 1), c.bootstrap_workspace_bytes(plan, cts, stc, True, 1)
    raised = 2 * (plan.cts_level + 1) * N * 8
    assert with_keys >= without + raised > raised + 6 * N * 8
    assert c.bootstrap_workspace_bytes(plan, cts, stc, False, 2) > without
    assert c.bootstrap_workspace_bytes(plan, cts[:2], stc, False, 1) == 0 and c.bootstrap_workspace_bytes(plan, cts, stc, False, 0) == 0
    assert 2 * N - 1 in elts and all(e % 2 == 1 and 0 < e < 2 * N for e in elts)


def test_refusals_need_no_device(setup):
    c, primes, plan, cts, stc, key, elts = setup
    Q = c.Q_size
    room = 2 * (plan.out_level + 2) * N
    ct = torch.full((2 * N,), SENT, dtype=torch.int64)
    out = torch.full((room,), SENT, dtype=torch.int64)
    ws = torch.full((c.bootstrap_workspace_bytes(plan, cts, stc, True, 1) // 8,), SENT, dtype=torch.int64)

    def refused(text, **kw):
        args = dict(ct=ct, out=out, plan=plan, cts=cts, stc=stc, conj=key, relin=key, batch=1, ws=ws, d2s=key, s2d=key)
        args.update(kw)
        with pytest.raises(hg.HEError) as e:
            c.ckks_bootstrap(args["ct"], 2 * N, args["out"], room, args["plan"], args["cts"], args["stc"], args["conj"],
                             args["relin"], args["batch"], args["ws"], swk_dense_to_sparse=args["d2s"],
                             swk_sparse_to_dense=args["s2d"], stream=0)
        assert e.value.code == hg.E_INVALID, e.value
        assert str(e.value) == f"[{hg.E_INVALID}] {text}"
        for t in (ct, out, ws):
            assert bool((t == SENT).all())

    refused("bootstrap: both switch keys (dense to sparse, sparse to dense) or neither", d2s=None)
    refused("bootstrap: both switch keys (dense to sparse, sparse to dense) or neither", s2d=None)
    refused("bootstrap: batch must be at least 1", batch=0)
    refused("bootstrap: batch must be at least 1", batch=-1)
    refused("bootstrap: at most 16383 items per call", batch=16384)
    refused("workspace too small", ws=ws[:ws.numel() - 1])
    refused("bootstrap: null argument", ws=None)
    refused("bootstrap: null argument", ct=None)
    refused("bootstrap: null argument", out=None)
    refused("bootstrap: null argument", conj=None)
    refused("bootstrap: null argument", relin=None)
    refused("bootstrap: as many factors as the plan has pieces", cts=cts[:2])
    refused("bootstrap: as many factors as the plan has pieces", stc=stc + stc[:1])
    refused("bootstrap: the raise goes to a level the context has", plan=hg.bootstrap_plan(primes[:Q] + [primes[Q - 1]], DELTA, Q, K=12))
    not_the_plan = "bootstrap: the EvalMod plan is not the one of the bootstrap plan"
    refused(not_the_plan, plan=hg.BootstrapPlan(plan.c, hg.eval_mod_plan(12, 30, 3, plan.eval_level, plan.eval_in_scale, 2.0 ** 49, primes[:Q])))
    refused(not_the_plan, plan=hg.BootstrapPlan(plan.c, hg.eval_mod_plan(12, 30, 2, plan.eval_level, plan.eval_in_scale, plan.eval_target_scale, primes[:Q])))
    # an earlier refusal wins: the factor count before the caller's pointers, those before the switch keys and the stride
    refused("bootstrap: as many factors as the plan has pieces", cts=cts[:2], ct=None, d2s=None)
    refused("bootstrap: null argument", ct=None, d2s=None, ws=ws[:1])
    both = torch.full((2 * N + room,), SENT, dtype=torch.int64)
    refused("bootstrap: out must not overlap ct", ct=both[:2 * N], out=both[2 * N - 1:2 * N - 1 + room])
    refused("bootstrap: the workspace must overlap neither out nor ct", out=ws[:room])
    bfv = hg.Context.from_bit_sizes(hg.BFV, N, [40, 40], [40], plain_modulus=65537, sec=hg.SEC_NONE)
    with pytest.raises(hg.HEError) as e:
        bfv.ckks_bootstrap(ct, 2 * N, out, room, plan, cts, stc, key, key, 1, ws, stream=0)
    assert e.value.code == hg.E_INVALID
    assert np.all(out.numpy().view(np.uint64) == SENT)
