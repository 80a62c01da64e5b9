// rns.hpp -- launchers for the RNS element-wise kernels (internal C++).
// Each launcher cites the reference kernel it replaces; layouts are the
// reference's limb-major planar layout: [part][limb][coeff] per ciphertext,
// ciphertexts of a batch `*_stride` elements apart.
#pragma once
#include "modarith.cuh"
#include "bfv_plain.cuh"

namespace hegpu {

// reference src/lib/kernel/addition.cu:10-47
hipError_t rns_addition(const u64* a, const u64* b, u64* out, const Mod* mods, int n_power,
                        int limbs, int parts, int batch, int op /*0 add,1 sub,2 neg*/,
                        hipStream_t st);

// addition with per-ciphertext strides: out[b] = a[b] + b_[b] over [parts][limbs][N]
// (addition.cu:10-21 as used by ckks/operator.cu:1149)
hipError_t rns_addition_strided(const u64* a, u64 sa, const u64* b, u64 sb, u64* out, u64 so, const Mod* mods,
                                int n_power, int limbs, int parts, int batch, hipStream_t st);

// reference multiplication.cu:102-126
hipError_t rns_cross_multiplication(const u64* in1, u64 s1, const u64* in2, u64 s2, u64* out,
                                    u64 so, const Mod* mods, int n_power, int decomp_size,
                                    int batch, hipStream_t st);

// reference switchkey.cu:11-59, 1558-1590, 1592-1619 (digit decomposition):
// out[y][i][n] = in[y][n] mod q_{map(i)},  map(i) = i < split ? i : i+level.
hipError_t rns_decompose(const u64* in, u64 in_stride, u64* out, u64 out_stride, const Mod* mods,
                         int n_power, int digits, int nmods, int split, int level, int batch,
                         hipStream_t st);

// mod_raise_kernel (reference src/lib/kernel/bootstrapping.cu:339-376, restated: that file does not compile here): the
// q_0 limb of each part, coefficient domain, lifted as a centred integer into q_0 .. q_{limbs-1}.  in [parts][1][N],
// out [parts][limbs][N] per item; limb 0 is the input, limb j of a negative value q_j - (|c| mod q_j) (q_j itself
// when that is 0).  out may not overlap in.
hipError_t rns_mod_raise(const u64* in, u64 in_stride, u64* out, u64 out_stride, const Mod* mods, int n_power, int limbs,
                         int parts, int batch, hipStream_t st);

// The integer pre-multiplier of the CKKS refresh: in [2][1][N] per item at q_0 -> k * in mod q_0, k < q_0,
// written to a (part p at a + p * a_part_stride) and, if b is given, to b [2][N] per item as well.  Canonical residues:
// what hegpu_ckks_constant_op (HEGPU_CONST_MUL) gives on one limb.
hipError_t rns_scale_q0(const u64* in, u64 in_stride, u64 k, u64* a, u64 a_part_stride, u64 a_stride, u64* b, u64 b_stride,
                        const Mod* mods, int n_power, int batch, hipStream_t st);

// reference switchkey.cu:61-285: out[c][y][n] = sum_i in[i][y][n]*key[i][c][kidx(y)][n].
// key strides use key_limbs (= Q' at depth 0); kidx(y) = (y < split) ? y : y + level
// (method I leveled: split = l, level = depth maps row l to the P limb; method II,
// switchkey.cu:287-398: rows >= l are the P limbs).
// the same for up to 4 keys sharing one read of the digits (hoisted rotations); result of key e at
// out + e * out_key_stride
hipError_t rns_keyswitch_mac_keys(const u64* in, u64 in_stride, const u64* const* keys, int key_count, u64* out,
                                  u64 out_stride, u64 out_key_stride, const Mod* mods, int n_power, int digits, int nmods,
                                  int key_limbs, int split, int level, int batch, hipStream_t st);
hipError_t rns_keyswitch_mac(const u64* in, u64 in_stride, const u64* key, u64* out, u64 out_stride,
                             const Mod* mods, int n_power, int digits, int nmods, int key_limbs,
                             int split, int level, int batch, hipStream_t st);

// reference switchkey.cu:872-927 / 985-1046 (method II digit -> Q~ fast base
// conversion with the float32 overflow estimate); out [d][rc][N]
hipError_t rns_base_conversion_DtoQtilde(const u64* in, u64 in_stride, u64* out, u64 out_stride, const Mod* mods,
                                         const u64* matrix, const u64* mi_inv, const u64* prod, const int* I_j,
                                         const int* I_location, int n_power, int d, int rc, int l, int level,
                                         int max_cnt /* widest digit */, int batch, hipStream_t st);

// One mod-down (division by the special primes, or by the last ciphertext prime in a rescale, with rounding) as the
// launchers below take it; Context::moddown / Context::rescale_moddown build it for a depth.  Host only: the kernels
// take the members as scalar arguments.
struct ModDown {
    const Mod* mods;                           // the Q' chain (DEVICE, like the three tables)
    const u64 *half, *half_mod, *last_q_modinv; // per divisor: half of it, that modulo each remaining limb, its inverse there
    int n_power;
    int Qp_cur, Q_cur;     // limbs per part of the input / of the result
    int first_Qp, first_Q; // the same at depth 0: the divisors are moduli first_Qp - 1, first_Qp - 2, ... (row widths of the tables)
    int P_size;            // number of divisors
};

// first half of the multi-prime mod-down in its NTT-domain form (context.cpp m2_md_*; ops.cpp ckks_moddown_multi)
hipError_t rns_moddown_multi_stage_one(const u64* in, u64 in_stride, u64* out, u64 out_stride, const ModDown& md,
                                       const u64* G, const u64* C, int batch, hipStream_t st);
// reference switchkey.cu:480-611 / 1222-1282 (mod-down by P_size primes);
// with_ct: 0 none, 1 both parts, 2 part 0 only
hipError_t rns_moddown_extended(const u64* in, u64 in_stride, const u64* ct, u64 ct_stride, u64* out, u64 out_stride,
                                const ModDown& md, int with_ct, int batch, hipStream_t st);

// reference switchkey.cu:400-478 (switchkey != 0: ct added to part 0 only)
hipError_t rns_divide_round_lastq(const u64* in, u64 in_stride, const u64* ct, u64 ct_stride, u64* out,
                                  u64 out_stride, const ModDown& md, int switchkey, int batch, hipStream_t st);

// reference switchkey.cu:678-705
hipError_t rns_moddown_stage_one(const u64* in, u64 in_stride, u64* out, u64 out_stride, const ModDown& md, int batch,
                                 hipStream_t st);

// reference switchkey.cu:707-771 (ct may alias out; in: Qp_cur limbs per part); with_ct: 0 none (rescale,
// switchkey.cu:792-815), 1 both parts, 2 part 0 only (switchkey variant)
hipError_t rns_moddown_stage_two(const u64* in_last, u64 last_stride, const u64* in, u64 in_stride, const u64* ct,
                                 u64 ct_stride, u64* out, u64 out_stride, const ModDown& md, int with_ct, int batch,
                                 hipStream_t st);

// reference switchkey.cu:1621-1813 (mod-down by P_size primes + Galois permute)
hipError_t rns_moddown_permute(const u64* in, u64 in_stride, const u64* in2, u64 in2_stride, u64* out, u64 out_stride,
                               const ModDown& md, int galois_elt, int batch, hipStream_t st);

// plain strided copy of `limbs` limbs x `parts` parts (switchkey.cu:776-790,
// bfv_duplicate's c0 copy)
// Galois automorphism b(X) = a(X^g) of `limbs` NTT-domain limbs per item (slot gather); out must not alias in
hipError_t rns_permute_ntt(const u64* in, u64 in_stride, u64* out, u64 out_stride, int galois_elt, int n_power,
                           int limbs, int batch, hipStream_t st);
hipError_t rns_copy_limbs(const u64* in, u64 in_part_stride, u64 in_stride, u64* out,
                          u64 out_part_stride, u64 out_stride, int n_power, int limbs, int parts,
                          int batch, hipStream_t st);

// out[b][d*(rc+1)][*] = in[b][d][*] for d < limbs: places NTT-domain limb d in
// the (digit d, modulus d) slot of a [l][rc][N] key-switch buffer
hipError_t rns_copy_diag(const u64* in, u64 in_stride, u64* out, u64 out_stride, int n_power, int limbs, int rc,
                         int batch, hipStream_t st);

// reference multiplication.cu cipherplain_multiply_accumulate_kernel as used by host/ckks/operator.cu:2843, for all giant
// steps of a baby-step/giant-step matrix-vector product in one launch: out entry j (at out + j * 2 limbs N, items
// out_stride apart) = sum_i diags[index[j][i]] (.) rot entry i, both parts.  rot: n1 <= 16 ciphertexts per item, entry i
// at rot + i * 2 limbs N (the layout of op_ckks_rotate_hoisted); diags: [n_diag][limbs][N]; index: HOST [n2][n1], -1 =
// absent (a row of -1 writes zeros), travels in the kernel arguments.  out must not overlap rot.
hipError_t rns_ckks_diag_mac(const u64* rot, u64 rot_stride, int n1, const u64* diags, int n_diag, const int* index,
                             int n2, u64* out, u64 out_stride, const Mod* mods, int n_power, int limbs, int batch,
                             hipStream_t st);
// out[item] = sum of terms[k][item] over [2][limbs][N] (addition.cu:10-21, `count` <= 16 terms in one pass); terms /
// strides: HOST arrays
hipError_t rns_ckks_sum_terms(const u64* const* terms, const u64* strides, int count, u64* out, u64 out_stride,
                              const Mod* mods, int n_power, int limbs, int batch, hipStream_t st);

// The real / imaginary boundary of CoeffToSlot / SlotToCoeff, one read of each input and one write of each output.
// x, xc, c0, c1: [2][in_limbs][N] per item; outputs [2][out_limbs][N], out_limbs <= in_limbs (the first out_limbs limbs of
// each part are kept).  psi_half: DEVICE, psi^(N/2) per modulus (Context::tab).  Outputs may overlap no input.
//   split: out0 = x + xc, out1 = div_i(x - xc)        (addition.cu:10-47 + cipher_div_by_i_kernel, multiplication.cu:469-495)
//   merge: out = c0 + mult_i(c1)                      (cipher_mult_by_i_kernel :441-467 + addition)
hipError_t rns_ckks_conj_split(const u64* x, u64 x_stride, const u64* xc, u64 xc_stride, u64* out0, u64* out1,
                               u64 out_stride, const u64* psi_half, const Mod* mods, int n_power, int in_limbs,
                               int out_limbs, int batch, hipStream_t st);
hipError_t rns_ckks_conj_merge(const u64* c0, u64 c0_stride, const u64* c1, u64 c1_stride, u64* out, u64 out_stride,
                               const u64* psi_half, const Mod* mods, int n_power, int in_limbs, int out_limbs, int batch,
                               hipStream_t st);
//   real:  out = x + xc, the split's out0 alone; out may be x itself (same stride, out_limbs == in_limbs), never xc
hipError_t rns_ckks_conj_real(const u64* x, u64 x_stride, const u64* xc, u64 xc_stride, u64* out, u64 out_stride,
                              const Mod* mods, int n_power, int in_limbs, int out_limbs, int batch, hipStream_t st);

// A leaf of the polynomial evaluator (evaluate_poly_from_polynomial_basis, ckks/operator.cu:4400-4484, in one pass):
// out[p] = (p == 0 ? w_0 : 0) + sum_k w_k * terms[k][p] over the first `limbs` limbs, p = 0, 1.  terms / strides /
// term_limbs / weights: HOST arrays of `count` <= 15 entries (count 0: the constant alone); term k has term_limbs[k] >=
// limbs limbs per part and is read in place.  weights: (re, im) pairs, the Gaussian integers round(re) + round(im) i.
// psi_half: DEVICE, psi^(N/2) per modulus.  out may overlap no term.  N >= 512.
hipError_t rns_ckks_weighted_sum(const u64* const* terms, const u64* strides, const int* term_limbs, const double* weights,
                                 int count, double w0_re, double w0_im, u64* out, u64 out_stride, const u64* psi_half,
                                 const Mod* mods, int n_power, int limbs, int batch, hipStream_t st);
// The tail of a Chebyshev power (gen_power, ckks/operator.cu:4355-4394, in one pass): out = 2 a - b over the first `limbs`
// limbs of both parts; b == nullptr: round(value) is subtracted from part 0 instead.  a / b have a_limbs / b_limbs >=
// limbs limbs per part.  out == a is allowed when a_limbs == limbs; out may overlap neither otherwise.
hipError_t rns_ckks_double_sub(const u64* a, u64 a_stride, int a_limbs, const u64* b, u64 b_stride, int b_limbs,
                               double value, u64* out, u64 out_stride, const Mod* mods, int n_power, int limbs, int batch,
                               hipStream_t st);

// Everything after the product of a logic gate in one pass (HELogicOperator<BFV / CKKS>, host/bfv/operator.cuh:1324-2230,
// host/ckks/operator.cuh:2333-3500: add, add, mod_drop copies, sub, negate and the plaintext add of an encoded one as
// separate launches): out = c0 * one * [part 0] + c1 * (a + b) + c2 * p over the first `limbs` limbs of both parts, with
// (c0, c1, c2) a row of AND (0,0,1) OR (0,1,-1) XOR (0,1,-2) NAND (1,0,-1) NOR (1,-1,1) XNOR (1,-1,2) NOT (1,-1,0).
// a / b / p: [2][a_limbs / b_limbs / p_limbs][N] per item, each >= limbs, read in place; a is not read when c1 == 0, p is
// nullptr exactly when c2 == 0 (NOT, which has no b either).  b_kind GATE_B_PLAIN: part 0 only; CKKS (bfv == false): NTT
// domain, b = [b_limbs][N] residues, one = round(scale_one) in every position; BFV: coefficient domain, b = [N] residues
// mod t entering as D(m) (bfv_plain.cuh, coeff_div = floor(Q / t) mod q_j on the DEVICE), one = D(1) on coefficient 0.
// out may be a or b itself (same stride) when that operand has exactly `limbs` limbs; it may overlap nothing otherwise.
// N >= 512.  hipErrorInvalidValue: limbs < 1, an input limb count below limbs, 2 * batch > 65535, coefficients that are
// no row of the table, operands that do not fit the row.
enum { GATE_B_NONE = 0, GATE_B_CIPHER = 1, GATE_B_PLAIN = 2 };
enum { LOGIC_AND = 0, LOGIC_OR = 1, LOGIC_XOR = 2, LOGIC_NAND = 3, LOGIC_NOR = 4, LOGIC_XNOR = 5, LOGIC_NOT = 6 };
// the row (c0, c1, c2) of a gate; false: no such gate
bool logic_gate_coefficients(int gate, int coeff[3]);
hipError_t rns_gate_combine(bool bfv, int c0, int c1, int c2, const u64* a, u64 a_stride, int a_limbs, const u64* b,
                            int b_kind, u64 b_stride, int b_limbs, const u64* p, u64 p_stride, int p_limbs,
                            double scale_one, const u64* coeff_div, const BfvPlainScale& ps, u64* out, u64 out_stride,
                            const Mod* mods, int n_power, int limbs, int batch, hipStream_t st);

struct BehzDev {
    const Mod* ibase;       // q_0..q_{Q-1}
    const Mod* obase;       // Bsk
    Mod m_tilde;
    Mod plain;
    u64 inv_prod_q_mod_m_tilde;
    u64 inv_prod_B_mod_m_sk;
    const u64* inv_m_tilde_mod_Bsk;
    const u64* prod_q_mod_Bsk;
    const u64* base_change_matrix_Bsk;
    const u64* base_change_matrix_m_tilde;
    const u64* inv_punctured_prod_mod_base_array;
    const u64* inv_prod_q_mod_Bsk;
    const u64* inv_punctured_prod_mod_B_array;
    const u64* base_change_matrix_q;
    const u64* base_change_matrix_msk;
    const u64* prod_B_mod_q;
    // merged constants (context.cpp): m_tilde * inv_punct_q[i], t * inv_punct_q[i] mod q_i;
    // inv_prod_q_mod_Bsk[i] * inv_punct_B[i] mod Bsk_i
    const u64* mtilde_inv_punct;
    const u64* t_inv_punct;
    const u64* invq_inv_punct_B;
    const u64* msk_mod_q; // m_sk mod q_i
    // rows with their trailing constant factors multiplied in (context.cpp), so that a row is ONE lazy 128-bit sum and
    // one reduction: fc_matrix[i][j] = base_change_matrix_Bsk[i][j] * inv_m_tilde_mod_Bsk[i], fc_c1[i] = prod_q_mod_Bsk[i]
    // * inv_m_tilde_mod_Bsk[i]  (mod Bsk_i);  ff_matrix[i][j] = -base_change_matrix_Bsk[i][j] * c_i, ff_tc[i] = t * c_i
    // with c_i = inv_prod_q_mod_Bsk[i] [* inv_punctured_prod_mod_B_array[i] for i < |B|]  (mod Bsk_i)
    // Every one of these also carries the factor 2^64 (mod its modulus) that the Montgomery reduction of the lazy
    // sum (redc128) divides out: ff_q_matrix = base_change_matrix_q, ff_msk_matrix = base_change_matrix_msk,
    // ff_prod_B / ff_neg_prod_B = prod_B_mod_q[i] / q_i - prod_B_mod_q[i], each times 2^64.
    const u64* fc_matrix;
    const u64* fc_c1;
    const u64* ff_matrix;
    const u64* ff_tc;
    const u64* ff_q_matrix;
    const u64* ff_msk_matrix;
    const u64* ff_prod_B;
    const u64* ff_neg_prod_B;
    int ibase_size, obase_size;
    int split; // rows of the base conversions over four wavefronts: 1 / 0 forced, -1 by launch size (option behz_split)
};

// Sum of the partial inner products of a digit-split ks_row_mac launch (KsMacArgs::splits): part p of split s sits in
// the digit buffer `buf` ([digit][rc][N] per item) at digit s * digits / splits + p; out[item][p][slot] = their sum
// modulo the modulus of the slot (mod_order as in the launch, NULL: slot k is modulus k).
hipError_t rns_sum_partials(const u64* buf, u64 buf_item_stride, u64* out, u64 out_item_stride, const Mod* mods,
                            const int* mod_order, int n_power, int digits, int rc, int splits, int batch,
                            hipStream_t st);

// reference multiplication.cu:10-100
hipError_t rns_fast_convertion(const u64* in1, u64 s1, const u64* in2, u64 s2, u64* out, u64 so,
                               const BehzDev& b, int n_power, int batch, hipStream_t st);
// reference multiplication.cu:128-272
hipError_t rns_fast_floor(const u64* in, u64 si, u64* out, u64 so, const BehzDev& b, int n_power,
                          int batch, hipStream_t st);

} // namespace hegpu
