"""CPU: the factors of the CKKS encoder's special FFT that CoeffToSlot / SlotToCoeff apply (host-only C-ABI entries
hegpu_encoding_transform_shape / _fill through heongpu_amd.api.encoding_transform_factors), against U computed from its
definition, and the strided baby-step/giant-step plan that evaluates them.

n = N/2, L = log2 n, zeta = exp(2 pi i / 2N); U[j][k] = zeta^(5^j k) = F_L ... F_1 B with B the bit reversal on L bits.
Forward factors (SlotToCoeff): applied in order to B v they give U v.  Inverse factors (CoeffToSlot): applied in order
to U w they give 1/2 B w (the half belongs to the real / imaginary split that follows).

Tolerance 1e-9 * max|w| * n: FP64 products of at most L <= 15 unit-modulus twiddles, round-off of order L 2^-52 per
entry and n terms per row; a wrong twiddle, offset or order gives an error of order 1."""
import numpy as np
import pytest

from heongpu_amd.api import encoding_transform_factors, linear_transform_plan

DEGREES = [64, 256, 4096]
PIECES = [2, 3, 5]


def bitrev(n):
    bits = n.bit_length() - 1
    j = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((j >> b) & 1) << (bits - 1 - b)
    return r


def u_times(N, w):
    """U w from the definition, for one vector [n] or several [n][m] (row by row: no dense matrix)"""
    n = N // 2
    root = np.exp(2j * np.pi * np.arange(2 * N) / (2 * N))
    g = np.array([pow(5, j, 2 * N) for j in range(n)], dtype=np.int64)
    k = np.arange(n, dtype=np.int64)
    w = np.asarray(w, dtype=np.complex128)
    out = np.empty(w.shape, dtype=np.complex128)
    for j in range(n):
        out[j] = root[(g[j] * k) % (2 * N)] @ w
    return out


def apply(piece, v):
    out = np.zeros_like(v)
    for k, d in zip(piece.offsets, piece.diagonals):
        out += d * np.roll(v, -k)
    return out


def dense(piece, n):
    m = np.zeros((n, n), dtype=np.complex128)
    t = np.arange(n)
    for k, d in zip(piece.offsets, piece.diagonals):
        m[t, (t + k) % n] += d
    return m


def vectors(n, seed):
    rng = np.random.default_rng(seed)
    units = [0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1] + [int(k) for k in rng.integers(0, n, 9)]
    vs = []
    for k in units:
        e = np.zeros(n, dtype=np.complex128)
        e[k] = 1
        vs.append(e)
    vs += [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(16)]
    return vs


@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("N", DEGREES)
def test_group_shape(N, pieces):
    n, L = N // 2, (N // 2).bit_length() - 1
    for inverse in (False, True):
        groups = encoding_transform_factors(N, inverse, pieces)
        assert len(groups) == pieces
        sizes = [g.stages for g in groups]
        assert sum(sizes) == L and sizes == sorted(sizes, reverse=True), sizes
        assert set(sizes) <= {L // pieces, -(-L // pieces)}, sizes
        done = 0
        for g in groups:
            first = L - done - g.stages + 1 if inverse else done + 1  # inverse starts at stage L, forward at stage 1
            assert g.stride == 1 << (first - 1), (g.stride, first)
            assert len(g.offsets) <= 2 ** (g.stages + 1) - 1
            assert len(g.offsets) == len(set(g.offsets)) == g.diagonals.shape[0] and g.diagonals.shape[1] == n
            assert all(k % g.stride == 0 and -n // 2 < k <= n // 2 for k in g.offsets), g.offsets
            assert all(abs(k) <= (2 ** g.stages - 1) * g.stride for k in g.offsets), g.offsets
            assert all(np.any(d != 0) for d in g.diagonals)
            done += g.stages


@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("N", DEGREES)
def test_forward_factors_give_u(N, pieces):
    n = N // 2
    groups = encoding_transform_factors(N, False, pieces)
    rev = bitrev(n)
    vs = vectors(n, N + pieces)
    want = u_times(N, np.stack(vs, axis=1))
    for col, v in enumerate(vs):
        y = v[rev]  # B v
        for g in groups:
            y = apply(g, y)
        err = np.max(np.abs(y - want[:, col]))
        assert err <= 1e-9 * np.max(np.abs(v)) * n, err


@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("N", DEGREES)
def test_inverse_factors_give_half_of_the_bit_reversed_input(N, pieces):
    n = N // 2
    groups = encoding_transform_factors(N, True, pieces)
    rev = bitrev(n)
    ws = vectors(n, 3 * N + pieces)
    start = u_times(N, np.stack(ws, axis=1))
    for col, w in enumerate(ws):
        y = start[:, col].copy()
        for g in groups:
            y = apply(g, y)
        err = np.max(np.abs(y - 0.5 * w[rev]))
        assert err <= 1e-9 * np.max(np.abs(w)) * n, err
    # the half is spread evenly: every group carries 2^(-1/pieces), so every non-zero entry of a group of g inverse
    # stages (each entry of a stage has modulus 1/2) has modulus 2^-g 2^(-1/pieces)
    for g in groups:
        mod = np.abs(g.diagonals[g.diagonals != 0])
        assert np.allclose(mod, 2.0 ** (-g.stages - 1.0 / pieces), rtol=1e-12, atol=0)


@pytest.mark.parametrize("N", [64, 256])
def test_dense_products(N):
    """the same two statements with dense matrices, where they are small"""
    n = N // 2
    rev = bitrev(n)
    B = np.zeros((n, n))
    B[np.arange(n), rev] = 1
    U = u_times(N, np.eye(n))
    for pieces in PIECES:
        fwd = np.eye(n, dtype=np.complex128)
        for g in encoding_transform_factors(N, False, pieces):
            fwd = dense(g, n) @ fwd
        assert np.max(np.abs(fwd @ B - U)) <= 1e-9 * n
        inv = np.eye(n, dtype=np.complex128)
        for g in encoding_transform_factors(N, True, pieces):
            inv = dense(g, n) @ inv
        assert np.max(np.abs(inv @ U - 0.5 * B)) <= 1e-9 * n


def test_bad_arguments_are_refused():
    from heongpu_amd import HEError
    for N, pieces in ((4096, 1), (4096, 6), (4096, 0), (4095, 3), (16, 5)):
        with pytest.raises(HEError):
            encoding_transform_factors(N, False, pieces)


@pytest.mark.parametrize("stride", [1, 8, 256])
def test_strided_plan_represents_every_offset_once(stride):
    slots, n1 = 2048, 4
    offsets = [stride * q for q in range(-7, 8)]
    plan = linear_transform_plan(offsets, slots, n1, stride=stride)
    distinct = sorted({k % slots for k in offsets})
    assert plan.n1 <= n1 and plan.n2 <= 16
    assert all(b % stride == 0 and 0 <= b < stride * n1 for b in plan.baby_shifts)
    assert all(g % (stride * n1) == 0 for g in plan.giant_shifts)
    seen = []
    for row, g in zip(plan.index, plan.giant_shifts):
        for at, b in zip(row, plan.baby_shifts):
            if at >= 0:
                assert (b + g) % slots == distinct[at]
                assert plan.pre_rotation[at] == -g
                seen.append(at)
    assert sorted(seen) == list(range(len(distinct)))
    if stride > 1:  # without the stride every offset is a giant step of its own and the baby steps do nothing
        flat = linear_transform_plan(offsets, slots, 1)
        assert flat.n1 == 1 and flat.n2 == len(distinct)


def test_strided_plan_reproduces_the_product():
    """a group of the real factorisation, evaluated the way hegpu_ckks_linear_transform evaluates it"""
    N = 4096
    n = N // 2
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    for inverse in (False, True):
        for g in encoding_transform_factors(N, inverse, 3):
            plan = linear_transform_plan(g.offsets, n, stride=g.stride)
            assert plan.n2 <= 8 and plan.n1 <= 8, (plan.n1, plan.n2)
            order = np.argsort([k % n for k in g.offsets])  # the plan numbers the diagonals by k mod slots
            packed = [np.roll(g.diagonals[order[p]], -plan.pre_rotation[p]) for p in range(len(order))]
            babies = [np.roll(v, -sh) for sh in plan.baby_shifts]
            out = np.zeros(n, dtype=np.complex128)
            for row, sh in zip(plan.index, plan.giant_shifts):
                inner = np.zeros(n, dtype=np.complex128)
                for at, b in zip(row, babies):
                    if at >= 0:
                        inner += packed[at] * b
                out += np.roll(inner, -sh)
            assert np.max(np.abs(out - apply(g, v))) <= 1e-12 * n


def test_default_stride_changes_nothing():
    slots = 2048
    diags = [0, 1, 2, 3, 5, 8, 13, 21, 100, 2047]  # tests/test_linear_transform_plan.py
    for n1 in (1, 4, 16, None):
        a, b = linear_transform_plan(diags, slots, n1), linear_transform_plan(diags, slots, n1, stride=1)
        assert a == b
        period = {None: 4}.get(n1, n1)
        for p, k in enumerate(diags):
            j, i = divmod(k, period)
            assert a.index[a.giant_shifts.index(j * period)][a.baby_shifts.index(i)] == p
            assert a.pre_rotation[p] == -j * period
    assert linear_transform_plan(diags, slots, 1).giant_shifts == diags
    assert linear_transform_plan([-1, 3], slots, 4) == linear_transform_plan([slots - 1, 3 + slots], slots, 4, 1)
    with pytest.raises(ValueError):
        linear_transform_plan([8, 12], slots, 4, stride=8)
