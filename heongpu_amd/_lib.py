"""ctypes binding of libhegpu.so (the C ABI declared in include/hegpu.h).

This is plumbing only: every function here forwards to a C entry point; there
is no Python/CPU fallback.  If the HIP library is missing the import fails
loudly, and any device call without a GPU returns HEGPU_E_NODEVICE.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhegpu.so")
# TESTS ONLY: tests/audit/run_audit.py binds the INSTRUMENTED build of the same sources (tests/audit/Makefile: every FP64
# operation checked against exact integer arithmetic).  Only that file name is accepted; nothing in the product sets it.
if os.environ.get("HEGPU_AUDIT_LIB"):
    if os.path.basename(os.environ["HEGPU_AUDIT_LIB"]) != "libhegpu_audit.so":
        raise ImportError("HEGPU_AUDIT_LIB must name tests/audit/lib/libhegpu_audit.so")
    LIB_PATH = os.environ["HEGPU_AUDIT_LIB"]

u64 = ctypes.c_uint64
u64p = ctypes.c_void_p  # device or host address passed as integer
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t
voidp = ctypes.c_void_p



class LinearFactor(ctypes.Structure):
    """hegpu_linear_factor: the matrix arguments of hegpu_ckks_linear_transform for one factor of a sequence"""
    _fields_ = [("diags", ctypes.c_void_p), ("n_diag", c_int), ("index", ctypes.POINTER(c_int)), ("n1", c_int), ("n2", c_int),
                ("baby_keys", ctypes.POINTER(ctypes.c_void_p)), ("baby_elts", ctypes.POINTER(c_int)),
                ("giant_keys", ctypes.POINTER(ctypes.c_void_p)), ("giant_elts", ctypes.POINTER(c_int)),
                ("giant_parent", ctypes.POINTER(c_int))]


class PolyStep(ctypes.Structure):
    """hegpu_poly_step: one step of a polynomial-evaluation plan (hegpu_poly_eval_plan_fill)"""
    _fields_ = [("kind", ctypes.c_int32), ("dst", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32),
                ("c", ctypes.c_int32), ("level", ctypes.c_int32), ("mul_level", ctypes.c_int32),
                ("rescale_first", ctypes.c_int32), ("rescale_after", ctypes.c_int32), ("n_terms", ctypes.c_int32),
                ("term_reg", ctypes.c_int32 * 15), ("scale", ctypes.c_double), ("tail_const", ctypes.c_double),
                ("w0", ctypes.c_double * 2), ("w", (ctypes.c_double * 2) * 15)]


class BootstrapConfig(ctypes.Structure):
    """hegpu_bootstrap_config: the inputs of hegpu_bootstrap_plan_fill"""
    _fields_ = [("scale", ctypes.c_double), ("message_ratio", ctypes.c_double), ("K", ctypes.c_int32),
                ("sine_degree", ctypes.c_int32), ("double_angle", ctypes.c_int32), ("cts_level", ctypes.c_int32),
                ("cts_pieces", ctypes.c_int32), ("eval_level", ctypes.c_int32), ("stc_level", ctypes.c_int32),
                ("stc_pieces", ctypes.c_int32)]


class BootstrapPlan(ctypes.Structure):
    """hegpu_bootstrap_plan: every level and scale label of the CKKS refresh"""
    _fields_ = [("k1", ctypes.c_uint64), ("cts_level", ctypes.c_int32), ("cts_pieces", ctypes.c_int32),
                ("eval_level", ctypes.c_int32), ("stc_level", ctypes.c_int32), ("stc_pieces", ctypes.c_int32),
                ("out_level", ctypes.c_int32), ("K", ctypes.c_int32), ("sine_degree", ctypes.c_int32),
                ("double_angle", ctypes.c_int32), ("reserved", ctypes.c_int32), ("raise_scale", ctypes.c_double),
                ("cts_scale", ctypes.c_double * 5), ("cts_label", ctypes.c_double * 5), ("eval_in_scale", ctypes.c_double),
                ("eval_target_scale", ctypes.c_double), ("eval_out_scale", ctypes.c_double), ("stc_in_scale", ctypes.c_double),
                ("stc_scale", ctypes.c_double * 5), ("stc_label", ctypes.c_double * 5), ("out_scale", ctypes.c_double)]


class SlimBootstrapConfig(ctypes.Structure):
    """hegpu_slim_bootstrap_config: the inputs of hegpu_slim_bootstrap_plan_fill"""
    _fields_ = [("scale", ctypes.c_double), ("ratio", ctypes.c_double), ("phase", ctypes.c_double),
                ("amplitude", ctypes.c_double), ("offset", ctypes.c_double), ("K", ctypes.c_int32), ("degree", ctypes.c_int32),
                ("double_angle", ctypes.c_int32), ("cts_level", ctypes.c_int32), ("cts_pieces", ctypes.c_int32),
                ("stc_pieces", ctypes.c_int32), ("arithmetic", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SlimBootstrapPlan(ctypes.Structure):
    """hegpu_slim_bootstrap_plan: every level and scale label of the slim, bit and gate refreshes"""
    _fields_ = [("in_level", ctypes.c_int32), ("stc_pieces", ctypes.c_int32), ("cts_level", ctypes.c_int32),
                ("cts_pieces", ctypes.c_int32), ("eval_level", ctypes.c_int32), ("out_level", ctypes.c_int32),
                ("K", ctypes.c_int32), ("degree", ctypes.c_int32), ("double_angle", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("stc_scale", ctypes.c_double * 5), ("stc_label", ctypes.c_double * 5),
                ("raise_scale", ctypes.c_double), ("cts_scale", ctypes.c_double * 5), ("cts_label", ctypes.c_double * 5),
                ("ratio", ctypes.c_double), ("phase", ctypes.c_double), ("amplitude", ctypes.c_double),
                ("offset", ctypes.c_double), ("eval_in_scale", ctypes.c_double), ("eval_target_scale", ctypes.c_double),
                ("eval_out_scale", ctypes.c_double), ("out_scale", ctypes.c_double)]


# (name, restype, argtypes) -- must list EVERY symbol of include/hegpu.h
SIGNATURES = [
    ("hegpu_last_error", ctypes.c_char_p, []),
    ("hegpu_version", ctypes.c_char_p, []),
    ("hegpu_context_create", c_int,
     [c_int, c_int, ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_int), c_int, u64, c_int,
      ctypes.POINTER(voidp)]),
    ("hegpu_context_create_default", c_int, [c_int, c_int, c_int, u64, c_int, ctypes.POINTER(voidp)]),
    ("hegpu_context_create_from_primes", c_int,
     [c_int, c_int, ctypes.POINTER(u64), c_int, c_int, u64, ctypes.POINTER(voidp)]),
    ("hegpu_validate_coeff_modulus_values", c_int, [c_int, ctypes.POINTER(u64), c_int, c_int, c_int]),
    ("hegpu_context_destroy", None, [voidp]),
    ("hegpu_context_upload", c_int, [voidp]),
    ("hegpu_context_clone", c_int, [voidp, ctypes.POINTER(voidp)]),
    ("hegpu_context_upload_device", c_int, [voidp, c_int]),
    ("hegpu_context_device", c_int, [voidp]),
    ("hegpu_broadcast_key", c_int, [ctypes.POINTER(voidp), c_int, ctypes.POINTER(voidp), c_size_t, ctypes.POINTER(voidp)]),
    ("hegpu_broadcast_bytes", c_int, [ctypes.POINTER(c_int), c_int, ctypes.POINTER(voidp), c_size_t, ctypes.POINTER(voidp),
                                      ctypes.POINTER(c_int)]),
    ("hegpu_last_broadcast_path", c_int, []),
    ("hegpu_context_set_option", c_int, [voidp, ctypes.c_char_p, c_int]),
    ("hegpu_context_get_option", c_int, [voidp, ctypes.c_char_p, ctypes.POINTER(c_int)]),
    ("hegpu_tfhe_context_set_option", c_int, [voidp, ctypes.c_char_p, c_int]),
    ("hegpu_context_int", ctypes.c_long, [voidp, ctypes.c_char_p]),
    ("hegpu_context_get", ctypes.c_long, [voidp, ctypes.c_char_p, voidp, ctypes.c_long]),
    ("hegpu_context_device_ptr", voidp, [voidp, ctypes.c_char_p]),
    ("hegpu_steps_to_galois_elt", c_int, [c_int, c_int, c_int]),
    ("hegpu_ntt", c_int, [voidp, c_int, u64p, u64p, c_int, c_int, c_int, c_int, voidp, voidp, voidp]),
    ("hegpu_GPU_NTT", c_int, [voidp, c_int, u64p, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_GPU_NTT_Inplace", c_int, [voidp, c_int, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_GPU_INTT", c_int, [voidp, c_int, u64p, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_GPU_INTT_Inplace", c_int, [voidp, c_int, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_GPU_NTT_Modulus_Ordered_Inplace", c_int, [voidp, c_int, u64p, c_int, c_int, c_int, c_int, voidp, voidp]),
    ("hegpu_GPU_NTT_Poly_Ordered_Inplace", c_int, [voidp, c_int, u64p, c_int, c_int, c_int, c_int, voidp, voidp]),
    ("hegpu_addition", c_int, [voidp, u64p, u64p, u64p, c_int, c_int, c_int, c_int, voidp]),
    ("hegpu_cross_multiplication", c_int,
     [voidp, c_int, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_cipher_broadcast", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, c_int, c_int, c_int, voidp]),
    ("hegpu_mod_raise", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_ckks_mod_raise", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_keyswitch_multiply_accumulate", c_int,
     [voidp, u64p, u64, u64p, u64p, u64, c_int, c_int, c_int, c_int, c_int, c_int, voidp]),
    ("hegpu_base_conversion_DtoQtilde", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq_permute", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq_leveled_stage_one", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq_leveled_stage_two", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_move_cipher_leveled", c_int, [voidp, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq_rescale", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_divide_round_lastq_extended", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_fast_convertion", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, voidp]),
    ("hegpu_fast_floor", c_int, [voidp, u64p, u64, u64p, u64, c_int, voidp]),
    ("hegpu_workspace_bytes", c_size_t, [voidp, c_int, c_int, c_int]),
    ("hegpu_ckks_multiply", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_ckks_relinearize_inplace", c_int, [voidp, u64p, u64, u64p, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_probe_ckks_relinearize", c_int,
     [voidp, u64p, u64, u64p, c_int, c_int, voidp, c_size_t, ctypes.c_uint, voidp]),
    ("hegpu_probe_ks_launch_forms", None, [u64p]),
    ("hegpu_ckks_rescale_inplace", c_int, [voidp, u64p, u64, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_ckks_apply_galois", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, c_int, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_ckks_rotate_hoisted", c_int,
     [voidp, u64p, u64, u64p, u64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(c_int), c_int, c_int, c_int, voidp,
      c_size_t, voidp]),
    ("hegpu_ckks_diag_mac", c_int,
     [voidp, u64p, u64, c_int, u64p, c_int, ctypes.POINTER(c_int), c_int, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_ckks_linear_transform_workspace_bytes", c_size_t, [voidp, c_int, c_int, c_int, c_int]),
    ("hegpu_ckks_linear_transform", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, c_int, ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(ctypes.c_void_p),
      ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(c_int), c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_giant_step_chain", c_int, [ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    ("hegpu_ckks_linear_transform_chained", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, c_int, ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(ctypes.c_void_p),
      ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int, c_int,
      voidp, c_size_t, voidp]),
    ("hegpu_encoding_transform_shape", c_int,
     [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    ("hegpu_encoding_transform_fill", c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), voidp]),
    ("hegpu_poly_eval_plan_size", c_int,
     [c_int, voidp, c_int, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(u64), c_int,
      ctypes.POINTER(c_int)]),
    ("hegpu_poly_eval_plan_fill", c_int,
     [c_int, voidp, c_int, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(u64), c_int,
      ctypes.POINTER(PolyStep), c_int]),
    ("hegpu_eval_mod_plan_size", c_int,
     [c_int, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(u64), c_int, ctypes.POINTER(c_int)]),
    ("hegpu_eval_mod_plan_fill", c_int,
     [c_int, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(u64), c_int, ctypes.POINTER(PolyStep),
      c_int]),
    ("hegpu_ckks_weighted_sum", c_int,
     [voidp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u64), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_double),
      c_int, ctypes.c_double, ctypes.c_double, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_ckks_double_sub", c_int,
     [voidp, u64p, u64, c_int, u64p, u64, c_int, ctypes.c_double, u64p, u64, c_int, c_int, voidp]),
    ("hegpu_ckks_poly_eval_workspace_bytes", c_size_t, [voidp, ctypes.POINTER(PolyStep), c_int, c_int, c_int]),
    ("hegpu_ckks_poly_eval", c_int,
     [voidp, u64p, u64, u64p, u64, ctypes.POINTER(PolyStep), c_int, u64p, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_ckks_conj_split", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_ckks_conj_merge", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_ckks_encoding_transform_workspace_bytes", c_size_t, [voidp, ctypes.POINTER(LinearFactor), c_int, c_int, c_int]),
    ("hegpu_ckks_coeff_to_slot", c_int,
     [voidp, u64p, u64, u64p, u64p, u64, ctypes.POINTER(LinearFactor), c_int, u64p, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_ckks_slot_to_coeff", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, u64, ctypes.POINTER(LinearFactor), c_int, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bootstrap_plan_fill", c_int,
     [ctypes.POINTER(BootstrapConfig), ctypes.POINTER(u64), c_int, ctypes.POINTER(BootstrapPlan)]),
    ("hegpu_ckks_bootstrap_workspace_bytes", c_size_t,
     [voidp, ctypes.POINTER(BootstrapPlan), ctypes.POINTER(PolyStep), c_int, ctypes.POINTER(LinearFactor), c_int,
      ctypes.POINTER(LinearFactor), c_int, c_int, c_int]),
    ("hegpu_ckks_bootstrap", c_int,
     [voidp, u64p, u64, u64p, u64, ctypes.POINTER(BootstrapPlan), ctypes.POINTER(PolyStep), c_int,
      ctypes.POINTER(LinearFactor), c_int, ctypes.POINTER(LinearFactor), c_int, u64p, u64p, u64p, u64p, c_int, voidp,
      c_size_t, voidp]),
    ("hegpu_eval_trig_plan_size", c_int,
     [c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double,
      ctypes.POINTER(u64), c_int, ctypes.POINTER(c_int)]),
    ("hegpu_eval_trig_plan_fill", c_int,
     [c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double,
      ctypes.POINTER(u64), c_int, ctypes.POINTER(PolyStep), c_int]),
    ("hegpu_slim_bootstrap_plan_fill", c_int,
     [ctypes.POINTER(SlimBootstrapConfig), ctypes.POINTER(u64), c_int, ctypes.POINTER(SlimBootstrapPlan)]),
    ("hegpu_ckks_conj_real", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, c_int, c_int, voidp]),
    ("hegpu_ckks_slim_bootstrap_workspace_bytes", c_size_t,
     [voidp, ctypes.POINTER(SlimBootstrapPlan), ctypes.POINTER(PolyStep), c_int, ctypes.POINTER(LinearFactor), c_int,
      ctypes.POINTER(LinearFactor), c_int, c_int]),
    ("hegpu_ckks_slim_bootstrap", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, u64, ctypes.POINTER(SlimBootstrapPlan), ctypes.POINTER(PolyStep), c_int,
      ctypes.POINTER(LinearFactor), c_int, ctypes.POINTER(LinearFactor), c_int, u64p, u64p, c_int, voidp, c_size_t, voidp]),
    ("hegpu_ckks_gate_combine", c_int,
     [voidp, c_int, u64p, u64, c_int, u64p, c_int, u64, c_int, u64p, u64, c_int, ctypes.c_double, u64p, u64, c_int, c_int,
      voidp]),
    ("hegpu_bfv_gate_combine", c_int, [voidp, c_int, u64p, u64, u64p, c_int, u64, u64p, u64, u64p, u64, c_int, voidp]),
    ("hegpu_ckks_logic_gate", c_int,
     [voidp, c_int, u64p, u64, u64p, c_int, u64, u64p, ctypes.c_double, u64p, u64, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bfv_logic_gate", c_int,
     [voidp, c_int, u64p, u64, u64p, c_int, u64, u64p, u64p, u64, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bfv_multiply", c_int, [voidp, u64p, u64, u64p, u64, u64p, u64, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bfv_relinearize_inplace", c_int, [voidp, u64p, u64, u64p, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bfv_apply_galois", c_int,
     [voidp, u64p, u64, u64p, u64, u64p, c_int, c_int, voidp, c_size_t, voidp]),
    ("hegpu_rng_create", c_int, [u64, ctypes.POINTER(voidp)]),
    ("hegpu_rng_create_seeded", c_int, [ctypes.c_char_p, ctypes.POINTER(voidp)]),
    ("hegpu_rng_create_from_entropy", c_int, [ctypes.POINTER(voidp)]),
    ("hegpu_drbg_block", c_int, [ctypes.c_char_p, u64, u64, ctypes.POINTER(ctypes.c_uint32)]),
    ("hegpu_rng_destroy", None, [voidp]),
    ("hegpu_generate_secret_key", c_int, [voidp, voidp, c_int, u64p, voidp, c_size_t, voidp]),
    ("hegpu_generate_public_key", c_int, [voidp, voidp, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_generate_relin_key", c_int, [voidp, voidp, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_generate_switch_key", c_int, [voidp, voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_generate_galois_key", c_int, [voidp, voidp, u64p, c_int, u64p, voidp, c_size_t, voidp]),
    ("hegpu_ckks_encrypt", c_int, [voidp, voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_ckks_decrypt", c_int, [voidp, u64p, u64p, c_int, u64p, voidp]),
    ("hegpu_bfv_encrypt", c_int, [voidp, voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_bfv_decrypt", c_int, [voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_mpc_public_key_share", c_int, [voidp, voidp, voidp, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_mpc_relin_key_share_round1", c_int, [voidp, voidp, voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_mpc_relin_key_share_round2", c_int, [voidp, voidp, u64p, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_mpc_galois_key_share", c_int, [voidp, voidp, voidp, u64p, c_int, u64p, voidp, c_size_t, voidp]),
    ("hegpu_mpc_accumulate", c_int, [voidp, ctypes.POINTER(ctypes.c_void_p), c_int, c_int, u64p, voidp]),
    ("hegpu_mpc_relin_key_finish", c_int, [voidp, ctypes.POINTER(ctypes.c_void_p), c_int, u64p, u64p, voidp]),
    ("hegpu_mpc_ckks_decrypt_share", c_int, [voidp, voidp, u64p, u64, u64p, c_int, u64p, c_int, voidp]),
    ("hegpu_mpc_ckks_decrypt_merge", c_int,
     [voidp, u64p, u64, ctypes.POINTER(ctypes.c_void_p), c_int, c_int, u64p, c_int, voidp]),
    ("hegpu_mpc_bfv_decrypt_share", c_int, [voidp, voidp, u64p, u64, u64p, u64p, c_int, voidp]),
    ("hegpu_mpc_bfv_decrypt_merge", c_int,
     [voidp, u64p, u64, ctypes.POINTER(ctypes.c_void_p), c_int, u64p, c_int, voidp, c_size_t, voidp]),
    ("hegpu_mpc_ckks_refresh_share", c_int,
     [voidp, voidp, voidp, u64p, u64, u64p, c_int, c_int, u64p, c_int, voidp, c_size_t, voidp]),
    ("hegpu_mpc_ckks_refresh_merge", c_int,
     [voidp, voidp, u64p, u64, ctypes.POINTER(ctypes.c_void_p), c_int, c_int, u64p, u64, c_int, voidp, c_size_t, voidp]),
    ("hegpu_mpc_bfv_refresh_share", c_int, [voidp, voidp, voidp, u64p, u64, u64p, u64p, c_int, voidp, c_size_t, voidp]),
    ("hegpu_mpc_bfv_refresh_merge", c_int,
     [voidp, voidp, u64p, u64, ctypes.POINTER(ctypes.c_void_p), c_int, u64p, u64, c_int, voidp, c_size_t, voidp]),
    ("hegpu_bfv_noise_rns", c_int, [voidp, u64p, u64p, u64p, voidp]),
    ("hegpu_bfv_plain_to_ntt", c_int, [voidp, u64p, u64p, voidp]),
    ("hegpu_negacyclic_shift", c_int, [voidp, u64p, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_ckks_constant_op", c_int, [voidp, c_int, u64p, ctypes.c_double, u64p, c_int, c_int, voidp]),
    ("hegpu_ckks_gaussian_integer_op", c_int,
     [voidp, c_int, u64p, ctypes.c_double, ctypes.c_double, u64p, c_int, c_int, voidp]),
    ("hegpu_ckks_mult_i", c_int, [voidp, u64p, u64p, c_int, c_int, c_int, voidp]),
    ("hegpu_cipherplain_multiplication", c_int, [voidp, u64p, u64p, u64p, c_int, voidp]),
    ("hegpu_bfv_plain_addsub", c_int, [voidp, u64p, u64p, u64p, c_int, voidp]),
    ("hegpu_bfv_multiply_plain", c_int, [voidp, u64p, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_bfv_encode", c_int, [voidp, voidp, c_int, u64p, voidp]),
    ("hegpu_ckks_encode", c_int, [voidp, voidp, c_int, ctypes.c_double, u64p, voidp, c_size_t, voidp]),
    ("hegpu_ckks_decode", c_int, [voidp, u64p, c_int, ctypes.c_double, voidp, voidp, c_size_t, voidp]),
    ("hegpu_ckks_encode_complex", c_int, [voidp, voidp, c_int, ctypes.c_double, u64p, voidp, c_size_t, voidp]),
    ("hegpu_ckks_decode_complex", c_int, [voidp, u64p, c_int, ctypes.c_double, voidp, voidp, c_size_t, voidp]),
    ("hegpu_ckks_encode_coeff", c_int, [voidp, voidp, c_int, ctypes.c_double, u64p, voidp]),
    ("hegpu_ckks_decode_coeff", c_int, [voidp, u64p, c_int, ctypes.c_double, voidp, voidp, c_size_t, voidp]),
    ("hegpu_ckks_encode_scalar", c_int, [voidp, ctypes.c_double, ctypes.c_double, u64p, voidp]),
    ("hegpu_bfv_decode", c_int, [voidp, u64p, u64p, voidp, c_size_t, voidp]),
    ("hegpu_tfhe_context_create", c_int, [ctypes.POINTER(voidp)]),
    ("hegpu_tfhe_context_destroy", None, [voidp]),
    ("hegpu_tfhe_context_int", ctypes.c_long, [voidp, ctypes.c_char_p]),
    ("hegpu_tfhe_prime", u64, [voidp]),
    ("hegpu_tfhe_prepare_bootkey", c_int, [voidp, u64p, u64p, voidp]),
    ("hegpu_tfhe_prepared_format", c_int, [voidp, u64p, c_int]),
    ("hegpu_tfhe_gate_precompute", c_int, [voidp, c_int, voidp, voidp, voidp, voidp, voidp, voidp, c_int, voidp]),
    ("hegpu_tfhe_bootstrapping", c_int, [voidp, voidp, voidp, u64p, voidp, voidp, c_int, voidp]),
    ("hegpu_tfhe_status", c_int, [voidp, voidp]),
    ("hegpu_tfhe_key_switching", c_int, [voidp, voidp, voidp, voidp, voidp, voidp, voidp, c_int, voidp]),
    ("hegpu_tfhe_generate_secret_key", c_int, [voidp, voidp, voidp, voidp, voidp]),
    ("hegpu_tfhe_generate_bootstrapping_key", c_int,
     [voidp, voidp, voidp, voidp, u64p, voidp, voidp, voidp, c_size_t, voidp]),
    ("hegpu_tfhe_encrypt", c_int, [voidp, voidp, voidp, voidp, c_int, voidp, voidp, voidp]),
    ("hegpu_tfhe_decrypt_phase", c_int, [voidp, voidp, voidp, voidp, c_int, voidp, voidp]),
    ("hegpu_tfhe_mux", c_int,
     [voidp, voidp, voidp, voidp, voidp, voidp, voidp, voidp, voidp, u64p, voidp, voidp, c_int, voidp, c_size_t,
      voidp]),
    ("hegpu_tfhe_gate", c_int,
     [voidp, c_int, voidp, voidp, voidp, voidp, voidp, voidp, u64p, voidp, voidp, c_int, voidp, c_size_t, voidp]),
]

_lib = None


def load():
    """Load libhegpu.so and type every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C heongpu_amd/csrc`.  There is no CPU fallback.")
    # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  It must
    # be the copy already in the process when libhegpu.so is loaded, otherwise
    # two HIP runtimes coexist and neither sees the other's device state.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib
