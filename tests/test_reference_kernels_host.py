"""CPU tests of oracle/_ref/libref_kernels.so (the reference's own kernel files behind oracle/ref_kernels_driver.cpp):

* the arithmetic of the stand-in header (oracle/ref_shim/gpuntt/common/modular_arith.cuh), called on the host through
  the refk_host_* probes, equals Python integers inside the Barrett domain and the oracle's o_* everywhere;
* every refk_* launch entry refuses, without a GPU, a buffer one word too short, a zero count and n_power 11 -- and, in
  the driver's dry run, accepts the exact lengths (so the refused call is refused for that one word);
* nothing under oracle/_ref/ is tracked.

The library exists where the tree was built next to the reference (oracle/ref_build.py).  A tree built without it has
no reference binaries at all and these tests skip; reference consumers without the library is a broken build and fails."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import ref_kernels as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def refk():
    if not rk.available():
        assert not rk.reference_binaries(), "oracle/_ref/ holds reference consumers but no libref_kernels.so"
        pytest.skip("built without the reference tree")
    L = rk.lib()
    L.refk_set_dry_run(1)
    yield L
    L.refk_set_dry_run(0)


# one prime per width the contexts use: q = 1 mod 2^17, found by the oracle's own generator
@pytest.fixture(scope="module")
def primes(oracle):
    L = oracle.lib()
    out = []
    for bits in (30, 36, 40, 50, 60, 61):
        arr = (ctypes.c_uint64 * 1)()
        assert L.o_generate_primes(65536, (ctypes.c_int * 1)(bits), 1, arr) == 0
        assert int(arr[0]).bit_length() == bits
        out.append(int(arr[0]))
    return out


def test_modulus_record_equals_the_oracles(refk, oracle, primes):
    """Modulus64(q) of the stand-in == o_mod(q) == {q, bit length, floor(2^(2 bit + 1) / q)}; 2^32 is BEHZ's m_tilde."""
    for q in primes + [1 << 32, 1032193, 65537]:
        got = (ctypes.c_uint64 * 3)()
        refk.refk_host_mod(q, got)
        m = oracle.lib().o_mod(q)
        bit = q.bit_length()
        assert [int(v) for v in got] == [int(m.value), int(m.bit), int(m.mu)] == [q, bit, (1 << (2 * bit + 1)) // q]


def test_add_sub_mult_reduce_on_edge_operands(refk, oracle, primes):
    """add / sub / mult / reduce_forced over 0, 1, q/2, q - 1, q, (2^64 - 1 for reduce_forced) and pseudo-random residues:
    equal to the oracle's o_* for every pair, and to Python integers wherever the operation is exact (add / sub of
    reduced operands; mult inside the Barrett domain a * b < 2^(2 bit)).  sub(q, 0) == q is the reference's
    non-canonical corner (multiplication.cu:185)."""
    O = oracle.lib()
    for q in primes:
        m = O.o_mod(q)
        bit = q.bit_length()
        edge = [0, 1, 2, q // 2, q // 2 + 1, q - 2, q - 1, q]
        rnd = [random.Random(q + i).randrange(q) for i in range(24)]
        vals = edge + rnd
        assert refk.refk_host_sub(q, 0, q) == q
        for a in vals:
            for w in (a, (1 << 64) - 1, (1 << 63) + a, q + a, 2 * q + 1):
                assert refk.refk_host_reduce_forced(w, q) == O.o_reduce_forced(w, ctypes.byref(m)) == w % q
            for b in vals:
                assert refk.refk_host_add(a, b, q) == O.o_add(a, b, ctypes.byref(m))
                assert refk.refk_host_sub(a, b, q) == O.o_sub(a, b, ctypes.byref(m))
                got = refk.refk_host_mult(a, b, q)
                assert got == O.o_mult(a, b, ctypes.byref(m))
                if a < q and b < q:
                    assert refk.refk_host_add(a, b, q) == (a + b) % q
                    assert refk.refk_host_sub(a, b, q) == (a - b) % q
                if a * b < (1 << (2 * bit)):
                    assert got == (a * b) % q, (q, a, b)
        # outside the domain (a 61-bit operand against a narrower modulus, cipher_broadcast_kernel's mult(1, x, q_i)):
        # only the oracle's restated sequence is the yardstick
        wide = (1 << 61) - 1
        assert refk.refk_host_mult(1, wide, q) == O.o_mult(1, wide, ctypes.byref(m))


def test_reduce_of_a_128_bit_value(refk, primes):
    """reduce({low, high}) == the 128-bit value mod q, for every word pattern (exact: the shift-in reduction has no
    domain): 0, 1, q - 1, q, 2^64 - 1 in either word."""
    for q in primes:
        words = [0, 1, q - 1, q, q + 1, (1 << 63), (1 << 64) - 1, 0x0123456789ABCDEF]
        for lo in words:
            for hi in words:
                assert refk.refk_host_reduce128(lo, hi, q) == ((hi << 64) | lo) % q, (q, lo, hi)


# ---------------------------------------------------------------- the argument checks of every launch entry
N_POWER = 12
N = 1 << N_POWER
FAKE = 0x1000  # a non-null address that is never dereferenced: the dry run returns before any launch


def _moddown_words(first_qp, p):
    return sum(first_qp - 1 - i for i in range(p))


def _examples():
    """entry -> (scalars, {buffer: exact number of words / entries the kernel's index range needs}); written from the
    reference's kernels (the line ranges the driver cites), independently of the driver's own sums"""
    Q, Qp, l, rc, P = 3, 5, 2, 4, 2
    md = dict(modulus=Qp, half=P, half_mod=_moddown_words(Qp, P), last_q_modinv=_moddown_words(Qp, P))
    ex = {
        "refk_addition": (dict(op=0, limbs=3, parts=2), dict(in1=6 * N, in2=6 * N, out=6 * N, modulus=3)),
        "refk_bfv_plain_addsub": (dict(sub=0, plain_mod=65537, Q_mod_t=5, upper_threshold=9, Q_size=3, cipher_size=2),
                                  dict(cipher=6 * N, plain=N, out=6 * N, modulus=3, coeffdiv_plain=3)),
        "refk_ckks_constant_op": (dict(op=2, value=3.0, limbs=3, parts=2), dict(out=6 * N, modulus=3, **{"in": 6 * N})),
        "refk_cross_multiplication": (dict(decomp_size=4), dict(in1=8 * N, in2=8 * N, out=12 * N, modulus=4)),
        "refk_fast_convertion": (dict(m_tilde=1 << 32, inv_prod_q_mod_m_tilde=7, ibase_size=2, obase_size=3),
                                 dict(in1=4 * N, in2=4 * N, out=20 * N, ibase=2, obase=3, inv_m_tilde_mod_Bsk=3,
                                      prod_q_mod_Bsk=3, base_change_matrix_Bsk=6, base_change_matrix_m_tilde=2,
                                      inv_punctured_prod_mod_base_array=2)),
        "refk_fast_floor": (dict(plain_modulus=65537, inv_prod_B_mod_m_sk=7, ibase_size=2, obase_size=3),
                            dict(out=6 * N, ibase=2, obase=3, inv_punctured_prod_mod_base_array=2, base_change_matrix_Bsk=6,
                                 inv_prod_q_mod_Bsk=3, inv_punctured_prod_mod_B_array=2, base_change_matrix_q=4,
                                 base_change_matrix_msk=2, prod_B_mod_q=2, **{"in": 15 * N})),
        "refk_threshold": (dict(upper_half_threshold=9, decomp_size=3),
                           dict(plain=N, out=3 * N, modulus=3, upper_half_increment=3)),
        "refk_cipherplain": (dict(decomp_size=3), dict(cipher=6 * N, plain=3 * N, out=6 * N, modulus=3)),
        "refk_ckks_mult_i": (dict(divide=0, limbs=3, parts=2),
                             dict(out=6 * N, ntt_table=2 * N + 2, modulus=3, **{"in": 6 * N})),
        "refk_ckks_gaussian_integer_op": (dict(op=1, limbs=3, parts=2),
                                          dict(real_rns=3, imag_rns=3, out=6 * N, ntt_table=2 * N + 2, modulus=3,
                                               **{"in": 6 * N})),
        "refk_cipher_broadcast": (dict(Q_size=Q, rns_mod_count=Qp), dict(out=Q * Qp * N, modulus=Qp, **{"in": Q * N})),
        "refk_cipher_broadcast_leveled": (dict(first_rns_mod_count=Qp, current_rns_mod_count=rc, current_decomp_count=l),
                                          dict(out=l * rc * N, modulus=Qp, **{"in": l * N})),
        "refk_cipher_broadcast_switchkey_leveled": (
            dict(first_rns_mod_count=Qp, current_rns_mod_count=rc, current_decomp_mod_count=l),
            dict(cipher=2 * l * N, out0=l * N, out1=l * rc * N, modulus=Qp)),
        "refk_ckks_duplicate": (dict(first_rns_mod_count=Qp, current_rns_mod_count=rc, current_decomp_mod_count=l),
                                dict(cipher=2 * l * N, out=l * rc * N, modulus=Qp)),
        "refk_bfv_duplicate": (dict(Q_size=Q, rns_mod_count=Qp),
                               dict(cipher=2 * Q * N, out1=Q * N, out2=Q * Qp * N, modulus=Qp)),
        "refk_keyswitch_multiply_accumulate": (dict(Q_tilda_size=Qp, digits=5),
                                               dict(key=10 * Qp * N, out=2 * Qp * N, modulus=Qp, **{"in": 5 * Qp * N})),
        "refk_keyswitch_multiply_accumulate_leveled": (
            dict(first_rns_mod_count=6, current_decomp_mod_count=3),
            dict(key=2 * 3 * 6 * N, out=2 * 4 * N, modulus=6, **{"in": 3 * 4 * N})),
        "refk_keyswitch_multiply_accumulate_leveled_method_II": (
            dict(first_rns_mod_count=Qp, current_decomp_mod_count=l, current_rns_mod_count=rc, digits=5, level=1),
            dict(key=10 * Qp * N, out=2 * rc * N, modulus=Qp, **{"in": 5 * rc * N})),
        "refk_divide_round_lastq": (dict(switchkey=0, decomp_mod_count=Q),
                                    dict(ct=2 * Q * N, out=2 * Q * N, modulus=Q + 1, half=1, half_mod=Q, last_q_modinv=Q,
                                         **{"in": 2 * (Q + 1) * N})),
        "refk_divide_round_lastq_extended": (
            dict(mode=1, Q_prime_size=Qp, Q_size=Q, first_Q_prime_size=Qp, first_Q_size=Q, P_size=P),
            dict(ct=2 * Q * N, out=2 * Q * N, **md, **{"in": 2 * Qp * N})),
        "refk_divide_round_lastq_permute": (
            dict(bfv=0, galois_elt=2 * N - 1, Q_prime_size=rc, Q_size=l, first_Q_prime_size=Qp, first_Q_size=Q, P_size=P),
            dict(in2=l * N, out=2 * l * N, **md, **{"in": 2 * rc * N})),
        "refk_divide_round_lastq_leveled_stage_one": (
            dict(first_decomp_count=Q, current_decomp_count=l),
            dict(out=2 * l * N, modulus=Q + 1, half=1, half_mod=l, **{"in": 2 * (l + 1) * N})),
        "refk_divide_round_lastq_leveled_stage_two": (
            dict(switchkey=0, current_decomp_count=l),
            dict(in_last=2 * l * N, ct=2 * l * N, out=2 * l * N, modulus=l, last_q_modinv=l, **{"in": (2 * l + 1) * N})),
        "refk_move_cipher_leveled": (dict(current_decomp_count=l), dict(out=(2 * l + 1) * N, **{"in": (2 * l + 1) * N})),
        "refk_divide_round_lastq_rescale": (
            dict(current_decomp_count=l),
            dict(in_last=2 * l * N, out=2 * l * N, modulus=l, last_q_modinv=l, **{"in": (2 * l + 1) * N})),
        "refk_negacyclic_shift": (dict(shift=2 * N - 1, limbs=3, parts=2), dict(out=6 * N, modulus=3, **{"in": 6 * N})),
    }
    return ex


def _call(name, scalars, lengths, **override):
    kw = dict(scalars)
    kw.update(n_power=N_POWER, stream=None)
    for i, (arg, ln) in enumerate(lengths.items()):
        kw[arg] = (FAKE + 0x100000 * i, ln)  # distinct addresses: negacyclic_shift refuses out == in
    kw.update(override)
    return rk.call(name, **kw)


def _dtoq_call(**override):
    """refk_base_conversion_DtoQtilde reads its host copies of I_j / I_location; digits {2, 1} of l = 3 limbs"""
    ij = (ctypes.c_int * 2)(2, 1)
    il = (ctypes.c_int * 2)(0, 2)
    l, qt, d = 3, 5, 2
    kw = dict(leveled=1, n_power=N_POWER, l=l, Q_tilda=qt, d=d, level=1, stream=None, I_j=FAKE, I_location=FAKE + 64, I_len=d,
              h_I_j=ctypes.addressof(ij), h_I_location=ctypes.addressof(il), mod_index=FAKE + 128, out=(FAKE, d * qt * N),
              modulus=(FAKE, qt + 1), matrix=(FAKE, 2 * qt + qt), Mi_inv=(FAKE, l), prod=(FAKE, d * qt))
    kw["in"] = (FAKE, l * N)
    kw.update(override)
    return rk.call("refk_base_conversion_DtoQtilde", **kw)


def test_every_launch_entry_is_described(refk):
    assert set(_examples()) | {"refk_base_conversion_DtoQtilde"} == set(rk.SIGNATURES)
    exported = subprocess.run(["nm", "-D", "--defined-only", rk.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if " T refk_" in ln}
    launch = names - {"refk_abi_version", "refk_set_dry_run", "refk_moduli_fill"} - {n for n in names if "_host_" in n}
    assert launch == set(rk.SIGNATURES), launch ^ set(rk.SIGNATURES)


@pytest.mark.parametrize("name", sorted(_examples()))
def test_launch_entry_refuses_short_buffers_zero_counts_and_small_degrees(refk, name):
    scalars, lengths = _examples()[name]
    assert _call(name, scalars, lengths) == rk.OK  # dry run: every check passed, nothing was launched
    for arg, ln in lengths.items():
        assert _call(name, scalars, lengths, **{arg: (FAKE + 0x7000000, ln - 1)}) == rk.E_RANGE, arg
        assert _call(name, scalars, lengths, **{arg: (0, ln)}) == rk.E_NULL, arg
    for arg, kind in rk.SIGNATURES[name]:
        if kind == "count":
            assert _call(name, scalars, lengths, **{arg: 0}) == rk.E_ARG, arg
            assert _call(name, scalars, lengths, **{arg: -1}) == rk.E_ARG, arg
    assert _call(name, scalars, lengths, n_power=11) == rk.E_ARG
    assert _call(name, scalars, lengths, n_power=17) == rk.E_ARG


def test_base_conversion_entry_checks_its_digit_tables(refk):
    """the digit -> Q~ conversion indexes with I_j / I_location: the entry walks the caller's host copies"""
    assert _dtoq_call() == rk.OK
    for arg in ("in", "out", "modulus", "matrix", "Mi_inv", "prod"):
        ptr, ln = dict(out=(FAKE, 2 * 5 * N), modulus=(FAKE, 6), matrix=(FAKE, 15), Mi_inv=(FAKE, 3), prod=(FAKE, 10),
                       **{"in": (FAKE, 3 * N)})[arg]
        assert _dtoq_call(**{arg: (ptr, ln - 1)}) == rk.E_RANGE, arg
    assert _dtoq_call(I_len=1) == rk.E_RANGE
    for arg in ("l", "Q_tilda", "d"):
        assert _dtoq_call(**{arg: 0}) == rk.E_ARG, arg
    assert _dtoq_call(n_power=11) == rk.E_ARG
    assert _dtoq_call(l=2) == rk.E_RANGE  # digit 1 starts at limb 2: outside an input of two limbs
    wide = (ctypes.c_int * 2)(21, 1)  # more than the 20 words of the kernel's partial[]
    assert _dtoq_call(h_I_j=ctypes.addressof(wide)) == rk.E_ARG
    assert _dtoq_call(leveled=0, level=1) == rk.E_ARG


def test_entry_specific_argument_rules(refk):
    ex = _examples()
    s, ln = ex["refk_divide_round_lastq_permute"]
    assert _call("refk_divide_round_lastq_permute", s, ln, galois_elt=2 * N + 1) == rk.E_ARG
    assert _call("refk_divide_round_lastq_permute", s, ln, galois_elt=4) == rk.E_ARG
    assert _call("refk_divide_round_lastq_permute", s, ln, P_size=16) == rk.E_ARG  # last_ct[15]
    s, ln = ex["refk_negacyclic_shift"]
    assert _call("refk_negacyclic_shift", s, ln, shift=2 * N) == rk.E_ARG
    assert _call("refk_negacyclic_shift", s, ln, out=(FAKE, 6 * N), **{"in": (FAKE, 6 * N)}) == rk.E_ARG  # in place
    s, ln = ex["refk_fast_convertion"]
    assert _call("refk_fast_convertion", s, ln, obase_size=64) == rk.E_ARG  # temp2[obase_size] of 64 words
    s, ln = ex["refk_divide_round_lastq_extended"]
    assert _call("refk_divide_round_lastq_extended", s, ln, mode=3) == rk.E_ARG
    primes = (ctypes.c_uint64 * 2)(65537, 1 << 62)
    stage = (ctypes.c_uint64 * 6)()
    fill = refk.refk_moduli_fill
    assert fill(ctypes.addressof(primes), 0, ctypes.addressof(stage), 6, FAKE, 2, None) == rk.E_ARG
    assert fill(ctypes.addressof(primes), 2, ctypes.addressof(stage), 5, FAKE, 2, None) == rk.E_RANGE
    assert fill(ctypes.addressof(primes), 2, ctypes.addressof(stage), 6, FAKE, 1, None) == rk.E_RANGE
    assert fill(ctypes.addressof(primes), 2, ctypes.addressof(stage), 6, FAKE, 2, None) == rk.E_ARG  # 2^62: no prime of a chain


def test_nothing_of_the_reference_build_is_tracked():
    r = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], capture_output=True, text=True)
    if r.returncode == 0:  # an exported tree without its history has nothing to list
        assert r.stdout.strip() == ""
