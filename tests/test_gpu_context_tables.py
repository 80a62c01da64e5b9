"""The context's public registry and its guards (csrc/context.cpp upload(), csrc/cabi.cpp).

hegpu_context_device_ptr hands out the device copy of a host table by name: a name has a device pointer exactly when
the context built that host table, for every name the library uploads and for each kind of context (BFV, CKKS with
one special prime, CKKS with three).  A clone carries all thirteen options.  And an entry point called on a context
that has none of the tables it reads returns its error code and text -- it never reaches a kernel."""
import pytest

pytestmark = pytest.mark.gpu

# every table upload() puts on the device: 49 of 64-bit words, then 6 of 32-bit ints
DEVICE_TABLES = [
    "psi_half", "last_q_modinv", "half", "half_mod", "factor", "m2_md_W0", "m2_md_G", "m2_md_C",
    "rescaled_last_q_modinv", "rescaled_half_mod", "rescaled_half", "base_change_matrix_Bsk",
    "inv_punctured_prod_mod_base_array", "base_change_matrix_m_tilde", "inv_m_tilde_mod_Bsk", "prod_q_mod_Bsk",
    "inv_prod_q_mod_Bsk", "base_change_matrix_q", "base_change_matrix_msk", "inv_punctured_prod_mod_B_array",
    "behz_mtilde_inv_punct", "behz_t_inv_punct", "behz_invq_inv_punct_B", "behz_msk_mod_q", "behz_fc_matrix",
    "behz_fc_c1", "behz_ff_matrix", "behz_ff_tc", "behz_ff_q_matrix", "behz_ff_msk_matrix", "behz_ff_prod_B",
    "behz_ff_neg_prod_B", "prod_B_mod_q", "Mi", "Mi_inv", "upper_half_threshold", "decryption_modulus",
    "special_fft_roots_table", "special_ifft_roots_table", "coeff_div_plain_modulus", "upper_halfincrement", "Qi_t",
    "Qi_gamma", "Qi_inverse", "m2_Mi_inv", "m2_matrix", "m2_prod", "m2_matrix_mg", "m2_negprod_mg",
    "new_prime_locations", "new_input_locations", "m2_I_j", "m2_I_location", "encoding_location", "reverse_order",
]
# host tables that stay on the host (or reach the device inside an NTT plan), and names nobody builds
NOT_DEVICE_TABLES = ["modulus", "ntt_table", "intt_table", "n_inverse", "psi", "gamma", "Q_mod_t", "upper_threshold",
                     "base_Bsk", "q_Bsk_merge_modulus", "plain_ntt_tables", "no_such_table", "", "Half"]

OPTIONS = ["fused_row_mac", "fused_moddown", "col_multi", "single_pass", "ntt_galois", "galois_scatter", "fuse_inverse",
           "copy_along", "digit_split", "fp_ntt", "behz_split", "fused_tensor", "moddown_in_mac"]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _contexts(hg):
    n = 4096
    return {
        "bfv": hg.Context.from_default(hg.BFV, n, 1, 1032193),
        "ckks_p1": hg.Context.from_bit_sizes(hg.CKKS, n, [40, 30, 30], [40], sec=hg.SEC_NONE),
        "ckks_p3": hg.Context.from_bit_sizes(hg.CKKS, n, [36, 36, 36, 36], [37, 37, 37], sec=hg.SEC_NONE),
        "bfv_p2": hg.Context.from_bit_sizes(hg.BFV, n, [36, 36, 36], [37, 37], plain_modulus=1032193, sec=hg.SEC_NONE),
        "bfv_no_batching": hg.Context.from_default(hg.BFV, n, 1, 257),  # 2N does not divide t - 1
    }


def _has_table(c, name):
    try:
        c.table(name)
        return True
    except KeyError:
        return False


def test_device_registry_matches_host_tables(hg, torch):
    assert len(DEVICE_TABLES) == 55 and len(set(DEVICE_TABLES)) == 55
    seen = set()
    for kind, c in _contexts(hg).items():
        assert not any(c.device_ptr(name) for name in DEVICE_TABLES), (kind, "before upload")
        c.upload()
        ptrs = {}
        for name in DEVICE_TABLES:
            p = c.device_ptr(name)
            assert bool(p) == _has_table(c, name), (kind, name, p)
            if p:
                assert len(c.table(name)) > 0, (kind, name)
                ptrs[name] = p
                seen.add(name)
        assert len(set(ptrs.values())) == len(ptrs), (kind, "two names share a device table")
        for name in NOT_DEVICE_TABLES:
            assert not c.device_ptr(name), (kind, name)
        # what each kind of context has (the conditions the entry points check before they read a table)
        bfv, m2 = kind.startswith("bfv"), kind in ("ckks_p3", "bfv_p2")
        assert ("coeff_div_plain_modulus" in ptrs) == bfv and ("behz_fc_matrix" in ptrs) == bfv, kind
        assert ("rescaled_half" in ptrs) == (not bfv) and ("new_prime_locations" in ptrs) == (not bfv), kind
        assert ("m2_matrix_mg" in ptrs) == m2 and ("m2_md_W0" in ptrs) == m2 and ("m2_I_j" in ptrs) == m2, kind
        assert ("encoding_location" in ptrs) == (bfv and kind != "bfv_no_batching"), kind
        assert "half" in ptrs and "last_q_modinv" in ptrs and "psi_half" in ptrs and "factor" in ptrs, kind
    assert seen == set(DEVICE_TABLES)  # every name is exercised by at least one of the contexts


def test_clone_carries_every_option(hg, torch):
    non_default = {"fused_row_mac": 0, "fused_moddown": 0, "col_multi": 1, "single_pass": 0, "ntt_galois": 0,
                   "galois_scatter": 0, "fuse_inverse": 0, "copy_along": 0, "digit_split": 4, "fp_ntt": 0,
                   "behz_split": 1, "fused_tensor": 0, "moddown_in_mac": 0}
    assert sorted(non_default) == sorted(OPTIONS) and len(OPTIONS) == 13
    for kind in ("bfv", "ckks_p3"):
        c = _contexts(hg)[kind]
        for k, v in non_default.items():
            assert c.get_option(k) != v, (k, "is not a non-default value")
            c.set_option(k, v)
        d = c.clone()
        for k in OPTIONS:
            assert d.get_option(k) == c.get_option(k) == non_default[k], (kind, k)
        # the clone is a context of its own: same host tables, its own device tables, options no longer shared
        assert d.device == -1 and (d.Q_size, d.P_size, d.bsk_modulus) == (c.Q_size, c.P_size, c.bsk_modulus)
        assert [int(v) for v in d.table("modulus")] == [int(v) for v in c.table("modulus")]
        c.upload()
        d.upload()
        assert c.device_ptr("half") and d.device_ptr("half") and c.device_ptr("half") != d.device_ptr("half")
        with pytest.raises(hg.HEError) as e:  # fp_ntt decides the table layout: refused once uploaded
            d.set_option("fp_ntt", 1)
        assert e.value.code == hg.E_LOGIC
        d.set_option("col_multi", -1)
        assert (c.get_option("col_multi"), d.get_option("col_multi")) == (1, -1)


# (entry point, arguments after the context, kind of context, error code, text).  Every pointer is null: the call has
# to end at the check.  All of these checks exist unchanged since before the tables became typed members; the audit of
# the entry points against the tables they read found no path on which a missing table could reach a kernel.
P = None
WRONG_CONTEXT = [
    ("hegpu_divide_round_lastq", (P, 0, P, 0, P, 0, 0, 1, P), "ckks_p3", "E_LOGIC", "single special prime"),
    ("hegpu_divide_round_lastq", (P, 0, P, 0, P, 0, 0, 1, P), "bfv_p2", "E_LOGIC", "single special prime"),
    ("hegpu_divide_round_lastq_permute", (P, 0, P, 0, P, 0, 3, 1, 1, P), "bfv", "E_INVALID", "BFV ciphertexts have no depth"),
    ("hegpu_divide_round_lastq_extended", (P, 0, P, 0, P, 0, 0, 1, 1, P), "bfv", "E_INVALID", "BFV ciphertexts have no depth"),
    ("hegpu_divide_round_lastq_leveled_stage_one", (P, 0, P, 0, 1, 0, 1, P), "bfv", "E_INVALID", "CKKS context required"),
    ("hegpu_divide_round_lastq_leveled_stage_one", (P, 0, P, 0, 0, 0, 1, P), "ckks_p3", "E_LOGIC", "single special prime"),
    ("hegpu_divide_round_lastq_leveled_stage_two", (P, 0, P, 0, P, 0, P, 0, 0, 0, 1, P), "ckks_p3", "E_LOGIC", "single special prime"),
    ("hegpu_divide_round_lastq_leveled_stage_two", (P, 0, P, 0, P, 0, P, 0, 0, 0, 1, P), "bfv", "E_INVALID", "CKKS context required"),
    ("hegpu_divide_round_lastq_rescale", (P, 0, P, 0, P, 0, 0, 1, P), "bfv", "E_INVALID", "CKKS context required"),
    ("hegpu_base_conversion_DtoQtilde", (P, 0, P, 0, 0, 1, P), "ckks_p1", "E_LOGIC", "method II tables exist only when P_size > 1"),
    ("hegpu_base_conversion_DtoQtilde", (P, 0, P, 0, 0, 1, P), "bfv", "E_LOGIC", "method II tables exist only when P_size > 1"),
    ("hegpu_base_conversion_DtoQtilde", (P, 0, P, 0, 1, 1, P), "bfv_p2", "E_INVALID", "invalid depth"),
    ("hegpu_fast_convertion", (P, 0, P, 0, P, 0, 1, P), "ckks_p1", "E_INVALID", "BFV context required"),
    ("hegpu_fast_floor", (P, 0, P, 0, 1, P), "ckks_p1", "E_INVALID", "BFV context required"),
    ("hegpu_bfv_multiply", (P, 0, P, 0, P, 0, 1, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_relinearize_inplace", (P, 0, P, 1, P, 0, P), "ckks_p3", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_apply_galois", (P, 0, P, 0, P, 3, 1, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_encrypt", (P, P, P, P, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_decrypt", (P, P, P, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_noise_rns", (P, P, P, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_plain_addsub", (P, P, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_plain_to_ntt", (P, P, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_multiply_plain", (P, P, P, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_encode", (P, 0, P, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_decode", (P, P, P, 0, P), "ckks_p1", "E_INVALID", "context scheme mismatch"),
    ("hegpu_bfv_encode", (P, 0, P, P), "bfv_no_batching", "E_LOGIC", "batching needs a prime plain modulus"),
    ("hegpu_bfv_decode", (P, P, P, 0, P), "bfv_no_batching", "E_LOGIC", "batching needs a prime plain modulus"),
    ("hegpu_ckks_encode", (P, 0, 1.0, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_encode_complex", (P, 0, 1.0, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_encode_coeff", (P, 0, 1.0, P, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_encode_scalar", (1.0, 1.0, P, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_decode", (P, 0, 1.0, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_decode_complex", (P, 0, 1.0, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_decode_coeff", (P, 0, 1.0, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_encrypt", (P, P, P, P, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_decrypt", (P, P, 0, P, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_rescale_inplace", (P, 0, 0, 1, P, 0, P), "bfv", "E_INVALID", "context scheme mismatch"),
    ("hegpu_ckks_relinearize_inplace", (P, 0, P, 0, 1, P, 0, P), "bfv_p2", "E_INVALID", "context scheme mismatch"),
]


def test_wrong_kind_of_context_is_an_error_not_a_launch(hg, torch):
    from heongpu_amd import _lib
    lib = _lib.load()
    ctxs = _contexts(hg)
    for c in ctxs.values():
        c.upload()
    for fn, args, kind, code, text in WRONG_CONTEXT:
        rc = getattr(lib, fn)(ctxs[kind]._h, *args)
        msg = lib.hegpu_last_error().decode()
        assert rc == getattr(hg, code), (fn, kind, rc, msg)
        assert text in msg, (fn, kind, msg)
    torch.cuda.synchronize()
