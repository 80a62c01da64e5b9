"""hegpu_ckks_conj_real (rns.hip k_ckks_conj_real), N = 4096, chain {60, 60, 60 | 60}: out = x + xc on the
kept limbs of both parts.

Word for word it is hegpu_ckks_conj_split's out0 (launched on packed copies of the same inputs) and hegpu_addition on the
kept limbs.  Shapes: 3 limbs in, 3 and 2 out; batch 1 and 3.  Layouts (helpers.LAYOUTS, as tests/
test_gpu_operand_layout.py): packed, every operand 8 bytes off a 16-byte boundary, odd item strides, both.  Every
operand sits between sentinel words (the padding between items and the guard words in front and behind): none may
change, and the inputs stay as they were.  In place onto x is allowed when no limb is dropped and covered here; with a
dropped limb it is refused, nothing written."""
import numpy as np
import pytest

from helpers import LAYOUTS, items_of, laid_out, synth_ct

pytestmark = pytest.mark.gpu

N = 4096
L = 3


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_made = {}


def reference(hg, torch, out_limbs, batch):
    """context, inputs and the two references, once per shape"""
    from test_gpu_poly_eval import context
    if (out_limbs, batch) in _made:
        return _made[(out_limbs, batch)]
    c, primes = context(hg, [60, 60, 60], [60])
    Q = c.Q_size
    depth, out_depth = Q - L, Q - out_limbs
    xs = [synth_ct(primes, range(L), 2, N, 310 + b) for b in range(batch)]
    ys = [synth_ct(primes, range(L), 2, N, 320 + b) for b in range(batch)]
    words, ow = 2 * L * N, 2 * out_limbs * N
    x, y = hg.to_device(np.concatenate(xs)), hg.to_device(np.concatenate(ys))
    out0 = torch.zeros(batch * ow, dtype=torch.int64, device="cuda")
    out1 = torch.zeros(batch * ow, dtype=torch.int64, device="cuda")
    c.ckks_conj_split(x, words, y, words, out0, out1, ow, depth, out_depth, batch)
    added = []
    for b in range(batch):  # hegpu_addition on the kept limbs of both parts
        a = hg.to_device(np.ascontiguousarray(xs[b].reshape(2, L, N)[:, :out_limbs]).reshape(-1))
        k = hg.to_device(np.ascontiguousarray(ys[b].reshape(2, L, N)[:, :out_limbs]).reshape(-1))
        s = torch.empty_like(a)
        c.addition(a, k, s, out_limbs, 2, 1, op=0)
        added.append(s)
    torch.cuda.synchronize()
    split = hg.to_host(out0).reshape(batch, ow).copy()
    added = np.stack([hg.to_host(t) for t in added])
    assert np.array_equal(split, added)
    _made[(out_limbs, batch)] = (c, depth, out_depth, xs, ys, split)
    return _made[(out_limbs, batch)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("out_limbs", [3, 2])
def test_conj_real_is_the_split_s_real_half(hg, torch, out_limbs, batch, layout):
    c, depth, out_depth, xs, ys, want = reference(hg, torch, out_limbs, batch)
    lead, pad = LAYOUTS[layout]
    ow = 2 * out_limbs * N
    x, sx, x_ok = laid_out(xs, lead, pad)
    y, sy, y_ok = laid_out(ys, lead, pad)
    out, so, out_ok = laid_out([np.full(ow, 7, dtype=np.uint64) for _ in range(batch)], lead, pad)
    assert x.data_ptr() % 16 == 8 * lead and (pad % 2 == 0 or sx % 2 == 1)
    c.ckks_conj_real(x, sx, y, sy, out, so, depth, out_depth, batch)
    torch.cuda.synchronize()
    assert x_ok() and y_ok() and out_ok(), "written outside an operand"
    assert np.array_equal(items_of(x, sx, len(xs[0]), batch), np.stack(xs)), "x changed"
    assert np.array_equal(items_of(y, sy, len(ys[0]), batch), np.stack(ys)), "xc changed"
    got = items_of(out, so, ow, batch)
    assert np.array_equal(got, want), (out_limbs, batch, layout)
    assert batch == 1 or not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("layout", ["packed", "off8_odd"])
@pytest.mark.parametrize("batch", [1, 3])
def test_in_place_onto_x(hg, torch, batch, layout):
    c, depth, out_depth, xs, ys, want = reference(hg, torch, L, batch)
    lead, pad = LAYOUTS[layout]
    x, sx, x_ok = laid_out(xs, lead, pad)
    y, sy, y_ok = laid_out(ys, lead, pad)
    c.ckks_conj_real(x, sx, y, sy, x, sx, depth, depth, batch)
    torch.cuda.synchronize()
    assert x_ok() and y_ok()
    assert np.array_equal(items_of(y, sy, len(ys[0]), batch), np.stack(ys))
    assert np.array_equal(items_of(x, sx, len(xs[0]), batch), want)


def test_in_place_with_a_dropped_limb_is_refused(hg, torch):
    c, depth, out_depth, xs, ys, _ = reference(hg, torch, 2, 1)
    x, sx, x_ok = laid_out(xs, 0, 0)
    y, sy, _ = laid_out(ys, 0, 0)
    for out, so in ((x, sx), (x[N:], sx), (y, sy)):
        with pytest.raises(hg.HEError) as e:
            c.ckks_conj_real(x, sx, y, sy, out, so, depth, out_depth, 1)
        assert e.value.code == hg.E_INVALID
    torch.cuda.synchronize()
    assert x_ok() and np.array_equal(items_of(x, sx, len(xs[0]), 1), np.stack(xs))
    assert np.array_equal(items_of(y, sy, len(ys[0]), 1), np.stack(ys))
