"""An EvalMod plan (hegpu_eval_mod_plan_*) on the device: hegpu_ckks_poly_eval executes it, and the result is bit for bit
the same plan composed from the single entries (tests/test_gpu_poly_eval.py `compose`: multiply, relinearize, rescale,
gaussian_integer_op, constant_op, addition).

Two things in such a plan do not occur in a plan of hegpu_poly_eval_plan_*: the polynomial's last COMBINE, which rescales
its sum, is followed by further steps (its register holds the sum's limbs until the rescale compacts it), and the plan ends
with a POWER step, whose tail writes the result.  Both are covered here with r = 1, 2, 3 double angles; r = 0 is a plain
Chebyshev plan."""
import numpy as np
import pytest

from heongpu_amd import api
from helpers import synth_ct, synth_key
from test_gpu_poly_eval import LONG, N, SENTINEL, compose, context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("K,degree,r,depth,batch", [(2, 7, 2, 0, 2), (3, 12, 3, 0, 1), (2, 7, 1, 2, 2), (2, 5, 0, 3, 1),
                                                    (6, 15, 3, 0, 3)])
def test_eval_mod_plan_equals_the_step_by_step_composition(hg, torch, K, degree, r, depth, batch):
    c, primes = context(hg, *LONG)
    Q, Qp = c.Q_size, c.Q_prime_size
    l = Q - depth
    scale = float(primes[1])
    plan = hg.eval_mod_plan(K, degree, r, Q - 1 - depth, scale, scale, primes[:Q])
    kinds = [s.kind for s in plan.steps]
    assert kinds[len(kinds) - r:] == [api.POLY_POWER] * r and plan.level == Q - 1 - depth - int(degree).bit_length() - r
    if r:
        assert plan.steps[len(kinds) - r - 1].rescale_after == 1  # an inner step that rescales its sum
    ct = hg.to_device(np.concatenate([synth_ct(primes, range(l), 2, N, 7 * degree + b) for b in range(batch)]))
    key = hg.to_device(synth_key(primes, c.switch_key_digits(), Qp, N, 3))
    so = 2 * plan.out_limbs * N + 32
    out = torch.full((batch * so,), SENTINEL, dtype=torch.int64, device="cuda")
    nbytes = c.poly_eval_workspace_bytes(plan, depth, batch)
    assert nbytes > 0
    ws = torch.full((nbytes // 8 + 1,), SENTINEL, dtype=torch.int64, device="cuda")  # a guard word behind the workspace
    c.ckks_poly_eval(ct, 2 * l * N, out, so, plan, key, depth, batch, ws[:nbytes // 8])
    want = compose(c, hg, torch, plan, ct, key, depth, batch)
    torch.cuda.synchronize()
    words = 2 * (plan.level + 1) * N
    assert int(ws[-1].item()) == SENTINEL
    assert torch.equal(out.view(batch, so)[:, :words].contiguous().view(-1), want), (K, degree, r, depth, batch)
    assert bool((out.view(batch, so)[:, 2 * plan.out_limbs * N:] == SENTINEL).all()), "written past the result"


def test_a_bare_product_still_cannot_end_a_plan(hg, torch):
    """a POWER step without a tail leaves three parts in its register: refused as the last step, as before"""
    c, primes = context(hg, *LONG)
    Q = c.Q_size
    scale = float(primes[1])
    plan = hg.eval_mod_plan(2, 7, 1, Q - 1, scale, scale, primes[:Q])
    bad = type(plan.steps).from_buffer_copy(plan.steps)
    bad[len(bad) - 1].c = api.POLY_TAIL_NONE
    assert c.poly_eval_workspace_bytes(plan._replace(steps=bad), 0, 1) == 0
    ct = torch.zeros(2 * Q * N, dtype=torch.int64, device="cuda")
    out = torch.full((2 * plan.out_limbs * N,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = torch.empty(c.poly_eval_workspace_bytes(plan, 0, 1) // 8, dtype=torch.int64, device="cuda")
    with pytest.raises(hg.HEError) as e:
        c.ckks_poly_eval(ct, 2 * Q * N, out, 2 * plan.out_limbs * N, plan._replace(steps=bad), ct, 0, 1, ws)
    assert e.value.code == hg.E_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
