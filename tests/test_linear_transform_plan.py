"""The baby-step/giant-step plan of a plaintext matrix x encrypted vector product (heongpu_amd.api.linear_transform_plan,
host only): the plan is emulated on plain vectors with numpy.roll standing in for the rotations and compared with the
dense product.  A positive shift k moves slot s + k to slot s (tests/cpp/test_api.cpp: rotate_rows(1) shifts the slots
left by one), i.e. rot(k, x) = numpy.roll(x, -k)."""
import numpy as np
import pytest

from heongpu_amd.api import linear_transform_plan

SLOTS = 2048  # N = 4096
DIAGS = [0, 1, 2, 3, 5, 8, 13, 21, 100, 2047]


def rot(x, k):
    return np.roll(x, -k)


def dense(diags):
    m = np.zeros((SLOTS, SLOTS), dtype=np.complex128)
    s = np.arange(SLOTS)
    for k, d in diags.items():
        m[s, (s + k) % SLOTS] += d
    return m


def emulate(plan, diags, v):
    """what hegpu_ckks_linear_transform computes, on plain vectors"""
    ks = sorted(diags)
    packed = [rot(diags[k], plan.pre_rotation[p]) for p, k in enumerate(ks)]
    babies = [rot(v, sh) for sh in plan.baby_shifts]
    out = np.zeros(SLOTS, dtype=np.complex128)
    for row, g in zip(plan.index, plan.giant_shifts):
        inner = np.zeros(SLOTS, dtype=np.complex128)
        for at, b in zip(row, babies):
            if at >= 0:
                inner += packed[at] * b
        out += rot(inner, g)
    return out


@pytest.mark.parametrize("n1", [1, 4, 16, None])
def test_plan_reproduces_the_dense_product(n1):
    rng = np.random.default_rng(5)
    diags = {k: rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS) for k in DIAGS}
    v = rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS)
    if n1 == 1:  # a period of one makes every diagonal a giant step: ten fit, all of DIAGS' indices are kept
        plan = linear_transform_plan(DIAGS, SLOTS, 1)
        assert (plan.n1, plan.n2, plan.baby_shifts, plan.giant_shifts) == (1, 10, [0], DIAGS)
    else:
        plan = linear_transform_plan(DIAGS, SLOTS, n1)
    period = {None: 4}.get(n1, n1)  # ten diagonals: sqrt = 3.16, the nearest power of two is 4
    assert plan.n1 == len(plan.baby_shifts) <= period and plan.n2 == len(plan.giant_shifts) <= 16
    assert sorted(at for row in plan.index for at in row if at >= 0) == list(range(len(DIAGS)))
    for p, k in enumerate(DIAGS):
        j, i = divmod(k, period)
        assert plan.index[plan.giant_shifts.index(j * period)][plan.baby_shifts.index(i)] == p
        assert plan.pre_rotation[p] == -j * period
    assert np.allclose(emulate(plan, diags, v), dense(diags) @ v)


def test_negative_and_wrapping_indices_name_the_same_diagonal():
    assert linear_transform_plan([-1, 3], SLOTS, 4) == linear_transform_plan([SLOTS - 1, 3 + SLOTS], SLOTS, 4)


def test_default_period():
    for count, want in ((1, 1), (2, 1), (3, 2), (9, 4), (10, 4), (32, 4), (36, 8), (64, 8), (144, 16), (1000, 16)):
        ks = list(range(count))
        if -(-count // want) > 16:
            continue
        plan = linear_transform_plan(ks, SLOTS)
        assert plan.baby_shifts == list(range(min(want, count))), (count, want)


def test_more_than_sixteen_giant_steps_is_refused():
    linear_transform_plan(range(16 * 4), SLOTS, 4)          # 16 giant steps of 4: the most one transform holds
    with pytest.raises(ValueError):
        linear_transform_plan(range(16 * 4 + 1), SLOTS, 4)  # a 17th row
    with pytest.raises(ValueError):
        linear_transform_plan(range(0, 17 * 16, 16), SLOTS, 16)
    with pytest.raises(ValueError):
        linear_transform_plan(DIAGS, SLOTS, 17)
    with pytest.raises(ValueError):
        linear_transform_plan([], SLOTS)
