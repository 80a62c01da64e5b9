// ops.hpp -- batched operator sequences on a Context (internal C++).
#pragma once
#include "context.hpp"
#include "keygen.hpp"
#include "bootstrap_plan.hpp"
#include "poly_eval.hpp"

namespace hegpu {

enum { OP_CKKS_RELIN = 1, OP_CKKS_RESCALE = 2, OP_CKKS_GALOIS = 3, OP_BFV_MULTIPLY = 4, OP_BFV_RELIN = 5,
       OP_BFV_GALOIS = 6, OP_KEYGEN_SECRET = 7, OP_KEYGEN_PUBLIC = 8, OP_KEYGEN_SWITCH = 9, OP_CKKS_ENCRYPT = 10, OP_BFV_ENCRYPT = 11,
       OP_BFV_DECRYPT = 12, OP_BFV_DECODE = 13, OP_CKKS_ENCODE = 14,
       OP_CKKS_DECODE = 15, OP_BFV_MULTIPLY_PLAIN = 16, OP_CKKS_ROTATE_HOISTED = 17, OP_MPC_KEY_SHARE = 18,
       OP_MPC_BFV_DECRYPT_MERGE = 19, OP_MPC_REFRESH_SHARE = 20, OP_MPC_REFRESH_MERGE = 21, OP_CKKS_LOGIC_GATE = 22,
       OP_BFV_LOGIC_GATE = 23, OP_CKKS_MOD_RAISE = 25 /* 24 stays unassigned: include/hegpu.h */, OP_CKKS_BOOTSTRAP = 26 };

// Words of the workspace row `op` for `batch` items at `depth`.  Every shape is stated once, by a layout function of
// ops.cpp that this query and the sequence both read.
size_t ops_workspace_elems(const Context& c, int op, int depth, int batch);

hipError_t op_ckks_multiply(const Context& c, const u64* ct1, u64 s1, const u64* ct2, u64 s2, u64* out, u64 so,
                            int depth, int batch, hipStream_t st);
// Relinearize and apply_galois run key-switching method I with one special prime (P_size == 1), method II with several.
// `phases` (method I only): which launches of the sequence run (all by default; hegpu_probe_ckks_relinearize times them
// one by one)
enum { RELIN_PHASE_INTT_C2 = 1, RELIN_PHASE_COLUMN = 2, RELIN_PHASE_ROW_MAC = 4, RELIN_PHASE_INTT_P = 8,
       RELIN_PHASE_MODDOWN = 16, RELIN_PHASE_ALL = 31 };
hipError_t op_ckks_relinearize(const Context& c, u64* ct, u64 cs, const u64* key, int depth, int batch, u64* ws,
                               hipStream_t st, unsigned phases = RELIN_PHASE_ALL);
hipError_t op_ckks_rescale(const Context& c, u64* ct, u64 cs, int depth, int batch, u64* ws, hipStream_t st);
hipError_t op_ckks_apply_galois(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* key,
                                int galois_elt, int depth, int batch, u64* ws, hipStream_t st);
// The modulus raise of bootstrapping (mod_up_from_q0, ckks/operator.cu:3963-4033, without its key switches): ct [2][1][N]
// at q_0, NTT domain -> out [2][Q - out_depth][N], NTT domain, the centred lift of every coefficient.  out overlaps
// neither ct nor ws.  Workspace OP_CKKS_MOD_RAISE.
hipError_t op_ckks_mod_raise(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, int out_depth, int batch, u64* ws,
                             hipStream_t st);
hipError_t op_bfv_multiply(const Context& c, const u64* ct1, u64 s1, const u64* ct2, u64 s2, u64* out, u64 so,
                           int batch, u64* ws, hipStream_t st);
hipError_t op_bfv_relinearize(const Context& c, u64* ct, u64 cs, const u64* key, int batch, u64* ws,
                              hipStream_t st);
hipError_t op_bfv_apply_galois(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* key,
                               int galois_elt, int batch, u64* ws, hipStream_t st);

// fast_single_hoisting_rotation_ckks_method_I / _II (ckks/operator.cu:4674-5446): `count` rotations of one
// ciphertext with the decomposition and the digit NTT shared; keys / galois_elts are HOST arrays.  Workspace: the
// key-switch layout with `group` accumulators, OP_CKKS_GALOIS (group 1) or OP_CKKS_ROTATE_HOISTED (group 4);
// ops_rotate_hoisted_accumulators: the group a workspace of ws_elems words has room for.
int ops_rotate_hoisted_accumulators(const Context& c, int depth, int batch, size_t ws_elems);
hipError_t op_ckks_rotate_hoisted(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* const* keys,
                                  const int* galois_elts, int count, int depth, int batch, u64* ws, hipStream_t st,
                                  int group = 1);

// y = M v for a plaintext matrix given by its diagonals and an encrypted vector, baby-step/giant-step (the project's own
// entry; the reference's multiply_matrix, ckks/operator.cu:2803-2895, is private to its bootstrapping):
//   out = sum_j galois(giant_elts[j], sum_i diags[index[j][i]] (.) galois(baby_elts[i], ct))
// hoisted baby rotations -> one rns_ckks_diag_mac launch for all n2 inner sums -> one apply_galois per giant step with a
// non-zero element -> one k-way sum.  index / keys / elts: HOST arrays ([n2][n1], [n1], [n2]; element 0 = identity, its
// key is ignored).  Not rescaled.  Workspace: ops_linear_transform_workspace_elems, the same in both modes.
//
// Chained giant steps: giant_parent, a HOST array [n2], makes a forest of the terms (-1 = a root; nullptr
// or all -1 = the direct mode above, unchanged).  giant_elts[j] / giant_keys[j] are then term j's LINK, to its parent or,
// for a root, to the result:
//   S_j = inner_j + sum over the children k of j of galois(giant_elts[k], S_k),   out = sum over the roots r of
//   galois(giant_elts[r], S_r)
// deepest terms first, one op_ckks_apply_galois per link with a non-zero element and one rns_ckks_sum_terms per term with
// children (and one over the roots if there are several).  With host::giant_step_chain's table the links of one factor
// need two keys where the direct mode needs n2 - 1, for the same number of key switches.
// ops_giant_chain_check: nullptr, or what is wrong with the table (a parent outside [-1, n2), a term that is its own
// ancestor, a non-zero link element without a key).
size_t ops_linear_transform_workspace_elems(const Context& c, int n1, int n2, int depth, int batch);
const char* ops_giant_chain_check(const int* giant_parent, int n2, const u64* const* giant_keys, const int* giant_elts);
hipError_t op_ckks_linear_transform(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* diags,
                                    int n_diag, const int* index, int n1, int n2, const u64* const* baby_keys,
                                    const int* baby_elts, const u64* const* giant_keys, const int* giant_elts, int depth,
                                    int batch, u64* ws, hipStream_t st, const int* giant_parent = nullptr);

// ---- CoeffToSlot / SlotToCoeff (reference coeff_to_slot / slot_to_coeff, ckks/operator.cu:3566-3663,
// :3809-3891): a chain of op_ckks_linear_transform + op_ckks_rescale over the factors of the encoder's special FFT, and
// one pass at the real / imaginary boundary.  One factor = the arguments of op_ckks_linear_transform for one matrix, its
// diagonals encoded at the depth the chain has reached (depth + position, SlotToCoeff: + 1).
struct LinearFactor {
    const u64* diags;
    int n_diag;
    const int* index;
    int n1, n2;
    const u64* const* baby_keys;
    const int* baby_elts;
    const u64* const* giant_keys;
    const int* giant_elts;
    const int* giant_parent = nullptr; // chained giant steps: see op_ckks_linear_transform
};
// two ciphertexts of the start depth per item + the largest linear-transform workspace of the chain
size_t ops_encoding_transform_workspace_elems(const Context& c, const LinearFactor* f, int count, int depth, int batch);
// ct [2][l][N] -> count x (linear_transform, rescale) -> apply_galois(2N - 1) -> rns_ckks_conj_split into out0 / out1
// [2][l - count - 1][N]
hipError_t op_ckks_coeff_to_slot(const Context& c, const u64* ct, u64 cs, u64* out0, u64* out1, u64 so,
                                 const LinearFactor* f, int count, const u64* conj_key, int depth, int batch, u64* ws,
                                 hipStream_t st);
// c0, c1 [2][l][N] -> rns_ckks_conj_merge to depth + 1 -> count x (linear_transform, rescale); the last product is
// written to out and rescaled there: out holds [2][l - count][N] on the way, [2][l - count - 1][N] at the end
hipError_t op_ckks_slot_to_coeff(const Context& c, const u64* c0, u64 s0, const u64* c1, u64 s1, u64* out, u64 so,
                                 const LinearFactor* f, int count, int depth, int batch, u64* ws, hipStream_t st);

// ---- polynomial evaluation (reference evaluate_poly, ckks/operator.cu:4292-4671): executes a plan of
// host::poly_eval_plan and nothing else.  POWER: drop copy of the higher operand if the levels differ, op_ckks_multiply,
// op_ckks_relinearize, op_ckks_rescale, then (Chebyshev) one rns_ckks_double_sub.  LEAF: one rns_ckks_weighted_sum, every
// power read at its own level.  COMBINE: op_ckks_rescale of q if the plan says so, multiply and relinearize as above, one
// rns_ckks_sum_terms at the lower level, and the plan's final rescale.  Register 0 is ct at `depth`; the last step writes
// `out`, which needs room for [2][level + 1 + rescale_after][N] per item and holds [2][level + 1][N] on return.
// ops_poly_eval_check: nullptr, or what is wrong with the plan for this context and depth (registers, levels).
const char* ops_poly_eval_check(const Context& c, const host::PolyStep* plan, int n_steps, int depth);
// per item: every register at the limb count the plan gives it (a product without a tail: three parts at its product's
// level), one three-part product, one dropped copy, then the relinearize workspace at `depth`
size_t ops_poly_eval_workspace_elems(const Context& c, const host::PolyStep* plan, int n_steps, int depth, int batch);
hipError_t op_ckks_poly_eval(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const host::PolyStep* plan,
                             int n_steps, const u64* relin_key, int depth, int batch, u64* ws, hipStream_t st);

// ---- the CKKS refresh (reference regular_bootstrapping_v2, ckks/operator.cu:7147-7224): ct [2][1][N] per
// item at q_0 -> x k1 -> [apply_galois with the element 1 and swk_dense_to_sparse at depth Q - 1] -> op_ckks_mod_raise to
// the plan's cts_level -> [the same with swk_sparse_to_dense there] -> op_ckks_coeff_to_slot, its two halves as items
// [0, batch) and [batch, 2 batch) of one buffer -> ONE op_ckks_poly_eval of the EvalMod plan at batch 2 * batch ->
// op_ckks_slot_to_coeff.  out needs room for [2][out_level + 2][N] per item and holds [2][out_level + 1][N] on return, at
// the plan's out_scale.  Both switch keys or neither.  eval_mod: the steps of host::eval_mod_plan for the plan's
// (K, sine_degree, double_angle, eval_level, eval_in_scale, eval_target_scale).  cts / stc: the plan's piece counts.
// ops_bootstrap_check: nullptr, or what is wrong with the plan for this context.  Workspace: OP_CKKS_BOOTSTRAP is the head
// that depends on nothing but the batch; ops_bootstrap_workspace_elems is the whole (check first).
const char* ops_bootstrap_check(const Context& c, const host::BootstrapPlan& p, const host::PolyStep* eval_mod, int n_steps);
size_t ops_bootstrap_workspace_elems(const Context& c, const host::BootstrapPlan& p, const host::PolyStep* eval_mod,
                                     int n_steps, const LinearFactor* cts, const LinearFactor* stc, bool switch_keys, int batch);
hipError_t op_ckks_bootstrap(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const host::BootstrapPlan& p,
                             const host::PolyStep* eval_mod, int n_steps, const LinearFactor* cts, const LinearFactor* stc,
                             const u64* conj_key, const u64* relin_key, const u64* swk_dense_to_sparse,
                             const u64* swk_sparse_to_dense, int batch, u64* ws, hipStream_t st);

// ---- the slim family of refreshes (reference slim_bootstrapping, bit_bootstrapping, gate_bootstrapping):
// ct (and ct2 for a gate: their modular sum first, one addition launch into the workspace) [2][P_stc + 1][N] per item ->
// per SlotToCoeff factor op_ckks_linear_transform + op_ckks_rescale, down to q_0, no merge -> op_ckks_mod_raise to the
// plan's cts_level -> per CoeffToSlot factor the same -> op_ckks_apply_galois (2N - 1) -> rns_ckks_conj_real dropping one
// limb -> ONE op_ckks_poly_eval of the trig plan at batch `batch` into out ([2][out_level + 1 + rescale_after][N] of room).
// No switch keys.  trig: the steps of host::eval_trig_plan for the plan's (K, degree, double_angle, phase, amplitude, offset,
// eval_level, eval_in_scale, eval_target_scale).  The workspace has no row in the OP_* table: ops_slim_bootstrap_workspace_elems
// sizes all of it (check first).
const char* ops_slim_bootstrap_check(const Context& c, const host::SlimBootstrapPlan& p, const host::PolyStep* trig, int n_steps);
size_t ops_slim_bootstrap_workspace_elems(const Context& c, const host::SlimBootstrapPlan& p, const host::PolyStep* trig,
                                          int n_steps, const LinearFactor* cts, const LinearFactor* stc, int batch);
hipError_t op_ckks_slim_bootstrap(const Context& c, const u64* ct, u64 cs, const u64* ct2, u64 cs2, u64* out, u64 so,
                                  const host::SlimBootstrapPlan& p, const host::PolyStep* trig, int n_steps,
                                  const LinearFactor* cts, const LinearFactor* stc, const u64* conj_key, const u64* relin_key,
                                  int batch, u64* ws, hipStream_t st);

// ---- logic gates on bits held as 0 / 1 (HELogicOperator<CKKS / BFV>, host/ckks/operator.cuh:2333-3500,
// host/bfv/operator.cuh:1324-2230): the product sequence of the arithmetic operator into the workspace, then ONE
// rns_gate_combine pass that reads a, b and the product in place and writes out (AND: the pass is its copy out of the
// workspace).  NOT is the pass alone.  b_kind: GATE_B_CIPHER (multiply, relinearize, CKKS: rescale) or GATE_B_PLAIN
// (CKKS: cipherplain product with b [l][N] per item, rescale; BFV: op_bfv_multiply_plain with b [N] per item); a plaintext
// shared by the batch has b_stride 0.  CKKS: a, b at `depth` (l = Q - depth limbs), out [2][l - 1][N] (NOT: [2][l][N]);
// BFV: everything [2][Q][N], coefficient domain.  Workspace OP_CKKS_LOGIC_GATE / OP_BFV_LOGIC_GATE: one three-part product
// per item and the largest workspace of the sequence.
// gate: LOGIC_* (rns.hpp)
hipError_t op_ckks_logic_gate(const Context& c, int gate, const u64* a, u64 as, const u64* b, int b_kind, u64 bs,
                              const u64* relin_key, double scale_one, u64* out, u64 so, int depth, int batch, u64* ws,
                              hipStream_t st);
hipError_t op_bfv_logic_gate(const Context& c, int gate, const u64* a, u64 as, const u64* b, int b_kind, u64 bs,
                             const u64* relin_key, u64* out, u64 so, int batch, u64* ws, hipStream_t st);

// ---- key generation / encryption / decryption, key-switch method I
// The generator state: every sampling call consumes one stream id of the DRBG (drbg.hpp).
struct Rng {
    DrbgKey seed{}; // 256-bit ChaCha20 key (drbg.hpp)
    u64 stream = 0;
};
// HEKeyGenerator::generate_secret_key_v2 (ckks/keygenerator.cu:85-160); sk [Q'][N], NTT domain
hipError_t op_gen_secret_key(const Context& c, Rng& r, int hamming_weight, u64* sk, u64* ws, hipStream_t st);
// generate_public_key (ckks/keygenerator.cu:167-240); pk [2][Q'][N]
hipError_t op_gen_public_key(const Context& c, Rng& r, const u64* sk, u64* pk, u64* ws, hipStream_t st);
// generate_relin_key_method_I (:242-324) / generate_galois_key_method_I (:415-560); key [Q][2][Q'][N];
// galois_elt == 0: relinearisation key; old_sk != nullptr (galois_elt == 0): generate_switch_key_method_I
// (:996-1095), the key under `sk` that carries old_sk
hipError_t op_gen_switch_key(const Context& c, Rng& r, const u64* sk, int galois_elt, const u64* old_sk, u64* key,
                             u64* ws, hipStream_t st);
// HEEncryptor<CKKS>::encrypt_ckks (ckks/encryptor.cu:36-110); plain [Q][N] NTT domain, ct [2][Q][N]
hipError_t op_ckks_encrypt(const Context& c, Rng& r, const u64* pk, const u64* plain, u64* ct, u64* ws,
                           hipStream_t st);
// HEDecryptor<CKKS>::decrypt_ckks (ckks/decryptor.cu:38-58); plain [l][N], l = Q - depth
hipError_t op_ckks_decrypt(const Context& c, const u64* ct, const u64* sk, int depth, u64* plain, hipStream_t st);
// the scalars of the BFV scaled plaintext, for every kernel that forms it
BfvPlainScale bfv_plain_scale(const Context& c);
// HEEncryptor<BFV>::encrypt_bfv (bfv/encryptor.cu:39-108); plain [N] mod t, ct [2][Q][N] coefficient domain
hipError_t op_bfv_encrypt(const Context& c, Rng& r, const u64* pk, const u64* plain, u64* ct, u64* ws,
                          hipStream_t st);
// HEDecryptor<BFV>::decrypt_bfv (bfv/decryptor.cu:36-120), coefficient-domain ciphertext; plain [N]
hipError_t op_bfv_decrypt(const Context& c, const u64* ct, const u64* sk, u64* plain, u64* ws, hipStream_t st);
// first half of HEDecryptor<BFV>::noise_budget_calculation (bfv/decryptor.cu:170-225):
// out [Q][N] = t * (c0 + c1*s) mod q_j, coefficient domain (the caller composes and takes the norm)
hipError_t op_bfv_noise_rns(const Context& c, const u64* ct, const u64* sk, u64* out, hipStream_t st);
// HEEncoder<BFV>::encode_bfv / decode_bfv (bfv/encoder.cu:48-95, 213-249): message [size <= N]
// int64 (negative values wrap mod t) -> plain [N]; plain [N] -> message [N].  ws: N words (decode).
hipError_t op_bfv_encode(const Context& c, const long long* message, int message_size, u64* plain, hipStream_t st);
hipError_t op_bfv_decode(const Context& c, const u64* plain, u64* message, u64* ws, hipStream_t st);
// HEOperator<BFV>::multiply_plain_bfv, coefficient-domain ciphertext (bfv/operator.cu:432-503)
hipError_t op_bfv_plain_to_ntt(const Context& c, const u64* plain, u64* out, hipStream_t st);
hipError_t op_bfv_multiply_plain(const Context& c, const u64* ct, const u64* plain, u64* out, u64* ws, hipStream_t st);
// HEEncoder<CKKS>::encode_ckks / encode_ckks_coeff / decode_ckks / decode_ckks_coeff (ckks/encoder.cu:100-690).
// encode mode: 0 real slots, 1 complex slots ((re, im) pairs), 2 coefficients (<= N), 3 `scalar` in every slot;
// decode mode: 0 real parts [N/2], 1 complex slots [N/2 pairs], 2 coefficients [N].
// message: device doubles; plain [Q - depth][N] NTT domain
hipError_t op_ckks_encode(const Context& c, int mode, const double* message, int message_size, double scalar,
                          double scale, u64* plain, u64* ws, hipStream_t st);
hipError_t op_ckks_decode(const Context& c, int mode, const u64* plain, int depth, double scale, double* message,
                          u64* ws, hipStream_t st);

// ---- N-out-of-N multiparty protocol (host/{ckks,bfv}/mpcmanager.cu).  crs: the generator all parties seed alike
// (draws the common `a`); r: the party's own (errors, u).  Shares have the layout of the key they sum to.
enum { MPC_LAYOUT_PUBLIC_KEY = 0, MPC_LAYOUT_GALOIS_KEY = 1, MPC_LAYOUT_RELIN_ROUND1 = 2, MPC_LAYOUT_RELIN_FINISH = 3 };
// digits of a key-switching key: Q (method I) or the depth-0 digit partition (method II)
int switch_key_digits(const Context& c);
// generate_public_key_stage1 (ckks/mpcmanager.cu:36-90): share [2][Q'][N] = (-(a*s_i + e_i), a)
hipError_t op_mpc_public_key_share(const Context& c, Rng& crs, Rng& r, const u64* sk, u64* share, u64* ws,
                                   hipStream_t st);
// u_out == nullptr: generate_galois_key_method_I / _II_stage_1 (:751-1308), today's Galois key with the common a
// (galois_elt != 0).  u_out != nullptr: generate_relin_key_method_I_stage_1 / _II_stage_1 (:121-229, :346-462), round 1 of the
// relinearisation key; u_out [Q'][N] receives the party's ephemeral secret u_i (NTT domain), needed again in round 2
// old_sk (single party only): the switching key that carries old_sk
hipError_t op_mpc_switch_key_share(const Context& c, Rng& crs, Rng& r, const u64* sk, int galois_elt, u64* u_out,
                                   u64* share, u64* ws, hipStream_t st, const u64* old_sk = nullptr);
// generate_relin_key_method_I_stage_3 / _II_stage_3 (:231-344, :464-582)
hipError_t op_mpc_relin_key_share_round2(const Context& c, Rng& r, const u64* sk, const u64* u, const u64* round1_sum,
                                         u64* share, u64* ws, hipStream_t st);
// generate_public_key_stage2, generate_relin_key_stage_2 / _stage_4, generate_galois_key_stage_2 (:92-119, :584-749,
// :1310-1481); shares: HOST array of k device pointers; round1_sum only for MPC_LAYOUT_RELIN_FINISH
hipError_t op_mpc_accumulate(const Context& c, const u64* const* shares, int k, int layout, const u64* round1_sum,
                             u64* out, hipStream_t st);
// partial_decrypt_stage_1 / _stage_2 (ckks/mpcmanager.cu:1483-1573, bfv/mpcmanager.cu:1440-1561); share
// [batch][Q - depth][N] (the h_i alone), plain [batch][Q - depth][N] (CKKS) or [batch][N] (BFV)
hipError_t op_mpc_ckks_decrypt_share(const Context& c, Rng& r, const u64* ct, u64 cs, const u64* sk, int depth,
                                     u64* share, int batch, hipStream_t st);
hipError_t op_mpc_bfv_decrypt_share(const Context& c, Rng& r, const u64* ct, u64 cs, const u64* sk, u64* share,
                                    int batch, hipStream_t st);
hipError_t op_mpc_ckks_decrypt_merge(const Context& c, const u64* ct, u64 cs, const u64* const* shares, int k,
                                     int depth, u64* plain, int batch, hipStream_t st);
hipError_t op_mpc_bfv_decrypt_merge(const Context& c, const u64* ct, u64 cs, const u64* const* shares, int k,
                                    u64* plain, int batch, u64* ws, hipStream_t st);

// distributed_bootstrapping_participant / _coordinator (ckks/mpcmanager.cu:1575-1903, bfv/mpcmanager.cu:1563-1752).
// Share: CKKS [batch][(Q - depth) + Q][N] NTT domain, BFV [batch][2][Q][N] coefficient domain; out [batch][2][Q][N]
// (CKKS: depth 0).  crs advances by one stream id per item (the common a: item b = the b-th draw of Q limbs), r by
// three per item (e0, e1, the mask): a batch draws what as many calls of one item draw.
// bit length of q_0 ... q_{l-1}
int level_modulus_bits(const Context& c, int l);
hipError_t op_mpc_ckks_refresh_share(const Context& c, Rng& crs, Rng& r, const u64* ct, u64 cs, const u64* sk,
                                     int depth, int mask_bits, u64* share, int batch, hipStream_t st);
hipError_t op_mpc_ckks_refresh_merge(const Context& c, Rng& crs, const u64* ct, u64 cs, const u64* const* shares,
                                     int k, int depth, u64* out, u64 so, int batch, u64* ws, hipStream_t st);
hipError_t op_mpc_bfv_refresh_share(const Context& c, Rng& crs, Rng& r, const u64* ct, u64 cs, const u64* sk,
                                    u64* share, int batch, hipStream_t st);
hipError_t op_mpc_bfv_refresh_merge(const Context& c, Rng& crs, const u64* ct, u64 cs, const u64* const* shares,
                                    int k, u64* out, u64 so, int batch, u64* ws, hipStream_t st);

} // namespace hegpu
