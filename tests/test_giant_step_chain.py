"""Chained giant steps on the host (heongpu_amd.api.giant_step_chain, hegpu_giant_step_chain), no GPU:

  1. the chain against a numpy model: folding the forest with numpy.roll over the plan's own pre-rotated diagonals gives
     M v within 1e-12 -- the rotations a term meets on its way to the result add up to its giant shift -- on the plans of
     tests/test_gpu_linear_transform.py, on a plan without a giant step 0 and with a gap, and on every factor of the
     special FFT at N = 2^12 (3 pieces) and N = 2^16 (4 pieces);
  2. every FFT factor has at most two distinct non-zero links, the chained key set is a subset of the direct one, and
     the counts of distinct rotation keys and of key switches are those of DESIGN.md's table;
  3. the rule itself on small examples, and the refusals, which need no device;
  4. the new struct field and the two new symbols.
"""
import ctypes
import functools

import numpy as np
import pytest

from heongpu_amd import _lib
from heongpu_amd.api import HEError, encoding_transform_factors, giant_step_chain, linear_transform_plan
from test_abi_struct_layout import CC, header_layout

SLOTS = 2048
DIAGS = [0, 1, 2, 3, 5, 8, 13, 21, 100, 2047]  # tests/test_gpu_linear_transform.py
PLANS = {"ten_diagonals_n1_4": (DIAGS, 4), "giant_steps_only": ([0, 1, 5, 2047], 1), "baby_steps_only": ([0, 1, 3], 4),
         "ten_diagonals_default": (DIAGS, None), "ten_diagonals_n1_1": (DIAGS, 1),
         "no_giant_zero_one_gap": ([5, 6, 9, 40, 41], 4)}


def rot(x, s):
    return np.roll(x, -s)


def fold(inner, parent, links):
    """S_j = inner_j + sum of rot(S_k, link_k) over the children k of j; the sum of rot(S_r, link_r) over the roots"""
    n2 = len(inner)

    def s(j):
        return inner[j] + sum(rot(s(k), links[k]) for k in range(n2) if parent[k] == j)

    return sum(rot(s(r), links[r]) for r in range(n2) if parent[r] == -1)


def check_plan(offsets, diagonals, plan, slots, rng):
    """offsets / diagonals: the matrix; the chained evaluation of `plan` against M v"""
    v = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    order = np.argsort([k % slots for k in offsets])  # the plan numbers the diagonals by k mod slots
    packed = [rot(diagonals[order[p]], plan.pre_rotation[p]) for p in range(len(order))]
    babies = [rot(v, s) for s in plan.baby_shifts]
    inner = [sum(packed[at] * babies[i] for i, at in enumerate(row) if at >= 0) + np.zeros(slots) for row in plan.index]
    want = sum(d * rot(v, k) for k, d in zip(offsets, diagonals))  # diag_k[t] = M[t][(t + k) mod slots]
    chain = giant_step_chain(plan.giant_shifts, slots)
    direct = sum(rot(inner[j], s) for j, s in enumerate(plan.giant_shifts))
    assert np.abs(direct - want).max() < 1e-12
    got = fold(inner, chain.parent, chain.link_shifts)
    err = np.abs(got - want).max()
    assert err < 1e-12, err
    return chain


@pytest.mark.parametrize("name", list(PLANS))
def test_fold_of_a_plan_is_the_matrix_product(name):
    ks, period = PLANS[name]
    rng = np.random.default_rng(len(name))
    diagonals = [rng.uniform(-1, 1, SLOTS) for _ in ks]
    plan = linear_transform_plan(ks, SLOTS, period)
    chain = check_plan(ks, diagonals, plan, SLOTS, rng)
    if name == "no_giant_zero_one_gap":
        assert plan.giant_shifts == [4, 8, 40]
        assert chain == ([-1, 0, 1], [4, 4, 32])  # the root carries its own shift, the gap a link of its own


@functools.lru_cache(maxsize=None)
def fft_factors(n, pieces):
    return [(inverse, g) for inverse in (True, False) for g in encoding_transform_factors(n, inverse, pieces)]


@pytest.mark.parametrize("n,pieces", [(4096, 3), (65536, 4)])
def test_fold_of_every_fft_factor_is_the_matrix_product(n, pieces):
    rng = np.random.default_rng(n)
    for inverse, g in fft_factors(n, pieces):
        plan = linear_transform_plan(g.offsets, n // 2, stride=g.stride)
        chain = check_plan(g.offsets, list(g.diagonals), plan, n // 2, rng)
        links = {s for s in chain.link_shifts if s}
        assert len(links) <= 2, (n, inverse, g.stride, sorted(links))
        assert sum(p == -1 for p in chain.parent) == 1  # the giant steps of a group are dense around 0: one tree


def key_sets(n, pieces, period=None):
    """(direct keys, chained keys, direct key switches, chained key switches) of CoeffToSlot + SlotToCoeff; the
    conjugation is not counted"""
    direct, chained, ks_direct, ks_chained = set(), set(), 0, 0
    for _inverse, g in fft_factors(n, pieces):
        plan = linear_transform_plan(g.offsets, n // 2, period, stride=g.stride)
        chain = giant_step_chain(plan.giant_shifts, n // 2)
        baby = {s for s in plan.baby_shifts if s}
        direct |= baby | {s for s in plan.giant_shifts if s}
        chained |= baby | {s for s in chain.link_shifts if s}
        ks_direct += len(baby) + sum(1 for s in plan.giant_shifts if s)
        ks_chained += len(baby) + sum(1 for s in chain.link_shifts if s)
    return direct, chained, ks_direct, ks_chained


# (N, pieces, period) -> distinct rotation keys direct, chained, key switches (the same in both modes)
KEY_COUNTS = {(65536, 4, None): (43, 26, 66), (65536, 4, 2): (66, 18, 100), (65536, 3, None): (38, 23, 76),
              (65536, 3, 4): (46, 15, 92), (4096, 3, None): (29, 18, 46)}


@pytest.mark.parametrize("case", list(KEY_COUNTS))
def test_key_counts_of_the_encoding_transforms(case):
    n, pieces, period = case
    direct, chained, ks_direct, ks_chained = key_sets(n, pieces, period)
    print(case, "direct", len(direct), "chained", len(chained), "key switches", ks_direct, ks_chained)
    assert (len(direct), len(chained), ks_direct) == KEY_COUNTS[case]
    assert ks_chained == ks_direct, "the chain costs no key switch"
    if period is None:
        assert chained <= direct, "whoever holds the direct keys holds the chained ones"


def test_the_rule_on_small_examples():
    # two-sided: the negative side hangs on the zero shift
    assert giant_step_chain([0, 4, 8, 2040, 2044], SLOTS) == ([-1, 0, 1, 4, 0], [0, 4, 4, SLOTS - 4, SLOTS - 4])
    # the order of the input does not matter to the tree, only to the numbering
    assert giant_step_chain([8, 2044, 0, 2040, 4], SLOTS) == ([4, 2, -1, 1, 2], [4, SLOTS - 4, 0, SLOTS - 4, 4])
    # no zero shift: two roots, each with its own shift
    assert giant_step_chain([4, 2044], SLOTS) == ([-1, -1], [4, 2044])
    # slots / 2 is positive: (-slots/2, slots/2]
    assert giant_step_chain([0, 1024, 1025], SLOTS) == ([-1, 0, 0], [0, 1024, 1025])
    assert giant_step_chain([7], SLOTS) == ([-1], [7])
    sixteen = giant_step_chain(list(range(16)), SLOTS)
    assert sixteen.parent == [-1] + list(range(15)) and sixteen.link_shifts == [0] + [1] * 15


@pytest.mark.parametrize("shifts,slots", [([], SLOTS), (list(range(17)), SLOTS), ([0, SLOTS], SLOTS), ([0, -1], SLOTS),
                                          ([0, 1], 3), ([0], 0)])
def test_refusals_need_no_device(shifts, slots):
    with pytest.raises(HEError) as e:
        giant_step_chain(shifts, slots)
    assert e.value.code == 10001, e.value  # HEGPU_E_INVALID


def test_null_arguments_are_refused():
    lib = _lib.load()
    one = (ctypes.c_int * 1)(0)
    assert lib.hegpu_giant_step_chain(None, 1, SLOTS, one, one) == 10001
    assert lib.hegpu_giant_step_chain(one, 1, SLOTS, None, one) == 10001
    assert lib.hegpu_giant_step_chain(one, 1, SLOTS, one, None) == 10001


def test_the_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("hegpu_giant_step_chain", "hegpu_ckks_linear_transform_chained"):
        assert hasattr(lib, name), name


@pytest.mark.skipif(CC is None, reason="no C compiler is installed")
def test_linear_factor_ends_with_the_parent_table(tmp_path):
    """giant_parent is the LAST field of hegpu_linear_factor, a pointer, and a factor zeroed by the caller is direct"""
    cls = _lib.LinearFactor
    fields = [f[0] for f in cls._fields_]
    assert fields[-1] == "giant_parent" and fields[:-1] == ["diags", "n_diag", "index", "n1", "n2", "baby_keys", "baby_elts",
                                                            "giant_keys", "giant_elts"]
    want = header_layout("hegpu_linear_factor", fields, tmp_path)
    got = [ctypes.sizeof(cls)]
    for f in fields:
        got += [getattr(cls, f).offset, getattr(cls, f).size]
    assert got == want
    assert cls.giant_parent.offset + cls.giant_parent.size == ctypes.sizeof(cls) and cls.giant_parent.size == ctypes.sizeof(ctypes.c_void_p)
    assert not cls().giant_parent
