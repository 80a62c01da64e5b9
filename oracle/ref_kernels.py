"""ctypes binding of oracle/_ref/libref_kernels.so: the reference's own RNS kernels behind the refk_* entries of
oracle/ref_kernels_driver.cpp (built by oracle/ref_build.py where the reference tree is available).

TEST INFRASTRUCTURE ONLY, like oracle/binding.py.  SIGNATURES is the one description of every launch entry: the tests
call through call(), and the CPU test of the argument checks walks the same table."""
import ctypes
import glob
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(REF_DIR, "libref_kernels.so")

OK, E_ARG, E_RANGE, E_NULL, E_LAUNCH = 0, -1, -2, -3, -4

# argument kinds: "i" int, "u" uint64, "d" double, "np" n_power, "count" an int that must be positive, "stream",
# "buf" a pointer followed by its length in 64-bit words, "mod" a Modulus64 array followed by its length in entries,
# "ptr" a bare pointer, "len" a bare length
SIGNATURES = {
    "refk_addition": [("op", "i"), ("in1", "buf"), ("in2", "buf"), ("out", "buf"), ("modulus", "mod"), ("n_power", "np"),
                      ("limbs", "count"), ("parts", "count"), ("stream", "stream")],
    "refk_bfv_plain_addsub": [("sub", "i"), ("cipher", "buf"), ("plain", "buf"), ("out", "buf"), ("modulus", "mod"),
                              ("plain_mod", "u"), ("Q_mod_t", "u"), ("upper_threshold", "u"), ("coeffdiv_plain", "buf"),
                              ("n_power", "np"), ("Q_size", "count"), ("cipher_size", "count"), ("stream", "stream")],
    "refk_ckks_constant_op": [("op", "i"), ("in", "buf"), ("value", "d"), ("out", "buf"), ("modulus", "mod"),
                              ("n_power", "np"), ("limbs", "count"), ("parts", "count"), ("stream", "stream")],
    "refk_cross_multiplication": [("in1", "buf"), ("in2", "buf"), ("out", "buf"), ("modulus", "mod"), ("n_power", "np"),
                                  ("decomp_size", "count"), ("stream", "stream")],
    "refk_fast_convertion": [("in1", "buf"), ("in2", "buf"), ("out", "buf"), ("ibase", "mod"), ("obase", "mod"),
                             ("m_tilde", "u"), ("inv_prod_q_mod_m_tilde", "u"), ("inv_m_tilde_mod_Bsk", "buf"),
                             ("prod_q_mod_Bsk", "buf"), ("base_change_matrix_Bsk", "buf"),
                             ("base_change_matrix_m_tilde", "buf"), ("inv_punctured_prod_mod_base_array", "buf"),
                             ("n_power", "np"), ("ibase_size", "count"), ("obase_size", "count"), ("stream", "stream")],
    "refk_fast_floor": [("in", "buf"), ("out", "buf"), ("ibase", "mod"), ("obase", "mod"), ("plain_modulus", "u"),
                        ("inv_punctured_prod_mod_base_array", "buf"), ("base_change_matrix_Bsk", "buf"),
                        ("inv_prod_q_mod_Bsk", "buf"), ("inv_punctured_prod_mod_B_array", "buf"),
                        ("base_change_matrix_q", "buf"), ("base_change_matrix_msk", "buf"), ("inv_prod_B_mod_m_sk", "u"),
                        ("prod_B_mod_q", "buf"), ("n_power", "np"), ("ibase_size", "count"), ("obase_size", "count"),
                        ("stream", "stream")],
    "refk_threshold": [("plain", "buf"), ("out", "buf"), ("modulus", "mod"), ("upper_half_increment", "buf"),
                       ("upper_half_threshold", "u"), ("n_power", "np"), ("decomp_size", "count"), ("stream", "stream")],
    "refk_cipherplain": [("cipher", "buf"), ("plain", "buf"), ("out", "buf"), ("modulus", "mod"), ("n_power", "np"),
                         ("decomp_size", "count"), ("stream", "stream")],
    "refk_ckks_mult_i": [("divide", "i"), ("in", "buf"), ("out", "buf"), ("ntt_table", "buf"), ("modulus", "mod"),
                         ("n_power", "np"), ("limbs", "count"), ("parts", "count"), ("stream", "stream")],
    "refk_ckks_gaussian_integer_op": [("op", "i"), ("in", "buf"), ("real_rns", "buf"), ("imag_rns", "buf"), ("out", "buf"),
                                      ("ntt_table", "buf"), ("modulus", "mod"), ("n_power", "np"), ("limbs", "count"),
                                      ("parts", "count"), ("stream", "stream")],
    "refk_cipher_broadcast": [("in", "buf"), ("out", "buf"), ("modulus", "mod"), ("n_power", "np"), ("Q_size", "count"),
                              ("rns_mod_count", "count"), ("stream", "stream")],
    "refk_cipher_broadcast_leveled": [("in", "buf"), ("out", "buf"), ("modulus", "mod"), ("first_rns_mod_count", "i"),
                                      ("current_rns_mod_count", "count"), ("n_power", "np"),
                                      ("current_decomp_count", "count"), ("stream", "stream")],
    "refk_cipher_broadcast_switchkey_leveled": [("cipher", "buf"), ("out0", "buf"), ("out1", "buf"), ("modulus", "mod"),
                                                ("n_power", "np"), ("first_rns_mod_count", "i"),
                                                ("current_rns_mod_count", "count"), ("current_decomp_mod_count", "count"),
                                                ("stream", "stream")],
    "refk_ckks_duplicate": [("cipher", "buf"), ("out", "buf"), ("modulus", "mod"), ("n_power", "np"),
                            ("first_rns_mod_count", "i"), ("current_rns_mod_count", "count"),
                            ("current_decomp_mod_count", "count"), ("stream", "stream")],
    "refk_bfv_duplicate": [("cipher", "buf"), ("out1", "buf"), ("out2", "buf"), ("modulus", "mod"), ("n_power", "np"),
                           ("Q_size", "count"), ("rns_mod_count", "count"), ("stream", "stream")],
    "refk_base_conversion_DtoQtilde": [("leveled", "i"), ("in", "buf"), ("out", "buf"), ("modulus", "mod"), ("matrix", "buf"),
                                       ("Mi_inv", "buf"), ("prod", "buf"), ("I_j", "ptr"), ("I_location", "ptr"),
                                       ("I_len", "len"), ("h_I_j", "ptr"), ("h_I_location", "ptr"), ("mod_index", "ptr"),
                                       ("n_power", "np"), ("l", "count"), ("Q_tilda", "count"), ("d", "count"),
                                       ("level", "i"), ("stream", "stream")],
    "refk_keyswitch_multiply_accumulate": [("in", "buf"), ("key", "buf"), ("out", "buf"), ("modulus", "mod"),
                                           ("n_power", "np"), ("Q_tilda_size", "count"), ("digits", "count"),
                                           ("stream", "stream")],
    "refk_keyswitch_multiply_accumulate_leveled": [("in", "buf"), ("key", "buf"), ("out", "buf"), ("modulus", "mod"),
                                                   ("first_rns_mod_count", "i"), ("current_decomp_mod_count", "count"),
                                                   ("n_power", "np"), ("stream", "stream")],
    "refk_keyswitch_multiply_accumulate_leveled_method_II": [
        ("in", "buf"), ("key", "buf"), ("out", "buf"), ("modulus", "mod"), ("first_rns_mod_count", "i"),
        ("current_decomp_mod_count", "count"), ("current_rns_mod_count", "count"), ("digits", "count"), ("level", "i"),
        ("n_power", "np"), ("stream", "stream")],
    "refk_divide_round_lastq": [("switchkey", "i"), ("in", "buf"), ("ct", "buf"), ("out", "buf"), ("modulus", "mod"),
                                ("half", "buf"), ("half_mod", "buf"), ("last_q_modinv", "buf"), ("n_power", "np"),
                                ("decomp_mod_count", "count"), ("stream", "stream")],
    "refk_divide_round_lastq_extended": [("mode", "i"), ("in", "buf"), ("ct", "buf"), ("out", "buf"), ("modulus", "mod"),
                                         ("half", "buf"), ("half_mod", "buf"), ("last_q_modinv", "buf"), ("n_power", "np"),
                                         ("Q_prime_size", "i"), ("Q_size", "count"), ("first_Q_prime_size", "i"),
                                         ("first_Q_size", "i"), ("P_size", "count"), ("stream", "stream")],
    "refk_divide_round_lastq_permute": [("bfv", "i"), ("in", "buf"), ("in2", "buf"), ("out", "buf"), ("modulus", "mod"),
                                        ("half", "buf"), ("half_mod", "buf"), ("last_q_modinv", "buf"), ("galois_elt", "i"),
                                        ("n_power", "np"), ("Q_prime_size", "i"), ("Q_size", "count"),
                                        ("first_Q_prime_size", "i"), ("first_Q_size", "i"), ("P_size", "count"),
                                        ("stream", "stream")],
    "refk_divide_round_lastq_leveled_stage_one": [("in", "buf"), ("out", "buf"), ("modulus", "mod"), ("half", "buf"),
                                                  ("half_mod", "buf"), ("n_power", "np"), ("first_decomp_count", "i"),
                                                  ("current_decomp_count", "count"), ("stream", "stream")],
    "refk_divide_round_lastq_leveled_stage_two": [("switchkey", "i"), ("in_last", "buf"), ("in", "buf"), ("ct", "buf"),
                                                  ("out", "buf"), ("modulus", "mod"), ("last_q_modinv", "buf"),
                                                  ("n_power", "np"), ("current_decomp_count", "count"), ("stream", "stream")],
    "refk_move_cipher_leveled": [("in", "buf"), ("out", "buf"), ("n_power", "np"), ("current_decomp_count", "count"),
                                 ("stream", "stream")],
    "refk_divide_round_lastq_rescale": [("in_last", "buf"), ("in", "buf"), ("out", "buf"), ("modulus", "mod"),
                                        ("last_q_modinv", "buf"), ("n_power", "np"), ("current_decomp_count", "count"),
                                        ("stream", "stream")],
    "refk_negacyclic_shift": [("in", "buf"), ("out", "buf"), ("modulus", "mod"), ("shift", "i"), ("n_power", "np"),
                              ("limbs", "count"), ("parts", "count"), ("stream", "stream")],
}

_CTYPES = {"i": [ctypes.c_int], "np": [ctypes.c_int], "count": [ctypes.c_int], "u": [ctypes.c_uint64],
           "d": [ctypes.c_double], "stream": [ctypes.c_void_p], "buf": [ctypes.c_void_p, ctypes.c_longlong],
           "mod": [ctypes.c_void_p, ctypes.c_longlong], "ptr": [ctypes.c_void_p], "len": [ctypes.c_longlong]}

_lib = None


def reference_binaries():
    """the reference consumers oracle/ref_build.py left under oracle/_ref/ (none: the tree was built without the reference)"""
    return sorted(glob.glob(os.path.join(REF_DIR, "ref_*")))


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = ctypes.CDLL(LIB_PATH)
    u64 = ctypes.c_uint64
    L.refk_host_mod.argtypes = [u64, ctypes.POINTER(u64)]
    L.refk_host_mod.restype = None
    for nm in ("refk_host_add", "refk_host_sub", "refk_host_mult", "refk_host_reduce128"):
        getattr(L, nm).argtypes = [u64, u64, u64]
        getattr(L, nm).restype = u64
    L.refk_host_reduce_forced.argtypes = [u64, u64]
    L.refk_host_reduce_forced.restype = u64
    L.refk_set_dry_run.argtypes = [ctypes.c_int]
    L.refk_set_dry_run.restype = None
    L.refk_moduli_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                   ctypes.c_longlong, ctypes.c_void_p]
    for name, sig in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [t for _, kind in sig for t in _CTYPES[kind]]
    _lib = L
    return L


def _pointer_and_length(value, kind):
    """a torch tensor of 64-bit words (length: its words, or its Modulus64 entries), a (pointer, length) pair, or None"""
    if value is None:
        return None, 0
    if isinstance(value, tuple):
        return value
    words = value.numel()
    return value.data_ptr(), words // 3 if kind == "mod" else words


def call(name, **kw):
    """refk_<name>(...) with the arguments by the names of SIGNATURES; returns the entry's code"""
    args = []
    for arg, kind in SIGNATURES[name]:
        v = kw.pop(arg)
        if kind in ("buf", "mod"):
            args += list(_pointer_and_length(v, kind))
        elif kind == "ptr":
            args.append(v if v is None or isinstance(v, int) else v.data_ptr())
        elif kind == "d":
            args.append(float(v))
        else:
            args.append(v)
    assert not kw, "unknown arguments %s" % sorted(kw)
    return getattr(lib(), name)(*args)
