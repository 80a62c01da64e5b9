/*
 * hegpu.h -- C ABI of the MI355X-native RNS-polynomial backend (libhegpu.so).
 *
 * The reference (Alisah-Ozcan/HEonGPU) has no FFI seam: its boundary is the
 * C++ class API plus, one level down, the gpuntt:: free functions and the
 * __global__ kernels of src/lib/kernel.  This header is that lower seam as a
 * plain C ABI: raw device pointers, sizes and a hipStream_t (as void*); no
 * torch or C++ types.  Every entry point cites the reference interface it
 * replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - all data is uint64 residues in the reference's limb-major planar layout:
 *    element [part][limb][coeff] of a ciphertext at
 *    coeff + (limb << n_power) + part * (limbs << n_power);
 *  - batched calls take `batch` ciphertexts `*_stride` ELEMENTS apart (batch == 0: nothing is launched, the call
 *    succeeds; batch < 0: an error);
 *  - operands (workspaces and keys included) need the alignment of their element type only, and any item stride not
 *    smaller than the item works, odd ones included.  Alignment to 16 bytes and even strides select the faster
 *    launch forms; results are identical either way;
 *  - every call is asynchronous on `stream`; return value 0 = success,
 *    otherwise a hipError_t code (or HEGPU_E_* below); hegpu_last_error()
 *    returns a message for the calling thread;
 *  - device pointers and the stream must belong to the device the context was uploaded to; the call runs there
 *    whatever the calling thread's current device is (see hegpu_context_upload_device).
 */
#ifndef HEGPU_H
#define HEGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hegpu_context hegpu_context; /* opaque */
typedef void* hegpu_stream;                 /* hipStream_t */

enum { HEGPU_BFV = 1, HEGPU_CKKS = 2 };
enum { HEGPU_SEC_NONE = 0, HEGPU_SEC_128 = 128, HEGPU_SEC_192 = 192, HEGPU_SEC_256 = 256 };
enum { HEGPU_TABLES_QP = 0, HEGPU_TABLES_Q_BSK = 1, HEGPU_TABLES_PLAIN = 2 /* BFV plain modulus t, batching */ };
enum {
    HEGPU_E_INVALID = 10001, /* std::invalid_argument in the reference */
    HEGPU_E_LOGIC = 10002,   /* std::logic_error */
    HEGPU_E_RUNTIME = 10003, /* std::runtime_error */
    HEGPU_E_NODEVICE = 10004
};

const char* hegpu_last_error(void);
const char* hegpu_version(void);

/* ------------------------------------------------------------------ context
 * HEContextImpl<S>: set_poly_modulus_degree + set_coeff_modulus_bit_sizes +
 * [set_plain_modulus] + generate  (src/lib/host/ckks/context.cu:33-147,272-440;
 * src/lib/host/bfv/context.cu:33-147,396-705).  Creation is host-only (works
 * without a GPU); hegpu_context_upload() puts the tables on the current
 * device.  Errors mirror the reference's exceptions. */
int hegpu_context_create(int scheme, int poly_modulus_degree, const int* log_q_bits, int q_count,
                         const int* log_p_bits, int p_count, uint64_t plain_modulus, int sec_level,
                         hegpu_context** out);
/* set_coeff_modulus_default_values(P_modulus_size) (bfv/context.cu:267-374) */
int hegpu_context_create_default(int scheme, int poly_modulus_degree, int p_count, uint64_t plain_modulus,
                                 int sec_level, hegpu_context** out);
/* set_coeff_modulus_values(Q, P) (bfv/context.cu:149-265): explicit primes */
int hegpu_context_create_from_primes(int scheme, int poly_modulus_degree, const uint64_t* primes, int q_count,
                                     int p_count, uint64_t plain_modulus, hegpu_context** out);
/* the checks set_coeff_modulus_values runs before it accepts explicit primes (bfv/context.cu:149-220: widths through
 * coefficient_validator, total width against the security table; plus that every value admits a 2N-th root of unity);
 * 0, or the reference's exception as a code + hegpu_last_error */
int hegpu_validate_coeff_modulus_values(int poly_modulus_degree, const uint64_t* primes, int q_count, int p_count,
                                        int sec_level);
void hegpu_context_destroy(hegpu_context* ctx);
/* Run-time options of a context (the reference configures through objects as well: ExecutionOptions,
 * src/include/heongpu/util/storagemanager.cuh:34-97; MemoryPoolConfig, util/memorypool.cuh:38-54).  They select
 * between forms of the same computation -- every setting gives bit-identical results -- and exist for measurements
 * and for the parity tests, which run each form.  -1 = chosen by launch size (the default of the tri-state ones).
 *   "fused_row_mac"  -1/0/1  key switch: row pass of the digit NTT fused with the key inner product / the
 *                            reference's kernel sequence (NTT of all digits, then keyswitch_multiply_accumulate)
 *   "fused_moddown"  0/1     mod-down stages as load transform / epilogue of the transform between them (1)
 *   "col_multi"      -1/0/1  decomposing column pass: one workgroup per source tile walking the target moduli
 *   "single_pass"    -1/0/1  N <= 2^14: one LDS-resident pass per transform instead of two
 *   "ntt_galois"     0/1     CKKS rotations without leaving the NTT domain (1) / in the reference's order
 *   "galois_scatter" 0/1     the NTT-domain automorphism as the mod-down epilogue's store (1) / a kernel of its own
 *   "fuse_inverse"   0/1     the inverse transform feeding a decomposition ends inside it (1)
 *   "copy_along"     0/1     rescale: the copy of the kept limbs rides on the column pass (1)
 *   "digit_split"    -1/0/2/4  workgroups per unit of the fused key switch for small launches
 *   "fp_ntt"         0/1     moduli below 2^50 on the exact FP64 butterflies (1); ONLY before hegpu_context_upload
 *                            (HEGPU_E_LOGIC afterwards: it decides the layout of the twiddle tables)
 *   "behz_split"     -1/0/1  BFV base conversions with their rows over four wavefronts
 *   "fused_tensor"   0/1     BFV multiply: the tensor product as the load transform of the inverse transform (1)
 *   "moddown_in_mac" 0/1     CKKS key switching with one special prime, fused path: the mod-down applied by the
 *                            inner-product kernels to their sums (1) / by the row pass of its own transform
 *   "wide_access"    0/1     fused key switch without digit splits: the inner-product kernels read the key, the
 *                            identity limb and the added ciphertext and write their results 16 bytes per lane (1) /
 *                            8 bytes per lane, the launches of the releases before the option (0)
 * Every option but "fp_ntt" may be changed at any time, but not concurrently with calls on the same context.  The
 * environment variables HEGPU_<NAME IN CAPITALS> seed the defaults once, when a context is created; no call path
 * reads the environment.  Unknown name / value out of range: HEGPU_E_INVALID. */
int hegpu_context_set_option(hegpu_context* ctx, const char* name, int value);
int hegpu_context_get_option(const hegpu_context* ctx, const char* name, int* value);
int hegpu_context_upload(hegpu_context* ctx);
/* ---- several GPUs in one process (batches of independent ciphertexts shard across the GPUs of a node,
 * only the evaluation keys are replicated).  One context per device: hegpu_context_clone copies the host-side
 * parameter set and options (not the device tables), hegpu_context_upload_device puts a context's tables on the
 * given device (hegpu_context_upload = the calling thread's current device).  Every entry point then runs on its
 * context's device whatever the caller's current device is (the caller's is restored on return), so a consumer drives
 * device d from any thread -- one OpenMP thread per device as the reference drives one stream per thread in
 * example/basic/9_multi_stream_usage_way1.cpp:27-66 -- with buffers and streams that belong to device d.
 * hegpu_broadcast_key copies keys[0] (on the device of ctxs[0]) to keys[i] on the device of ctxs[i], i = 1..n-1;
 * hegpu_broadcast_bytes is the same for any buffer (the TFHE boot and key-switch keys) with the devices given directly.
 * The copy into buffer i is ordered on streams[i] (NULL: the default streams), the source must be complete on
 * streams[0]'s timeline.  Path (hegpu_last_broadcast_path of the calling thread, or *path_out): peer access is
 * queried per edge (hipDeviceCanAccessPeer) and enabled (hipDeviceEnablePeerAccess); when every destination is
 * directly reachable from the source -- a fully connected xGMI node -- the copies are a FLAT fan-out, one hop, every
 * link of the source busy at once; otherwise a binomial TREE in <= 32 MiB chunks (hop r + 1 of a chunk starts when that
 * chunk has arrived).  HEGPU_BCAST_STAGED: at least one edge has no peer access and is staged through host memory by
 * the runtime; HEGPU_BCAST_SAME_DEVICE: every buffer lies on one device (a functional run on a 1-GPU box).
 * hegpu_context_device: -1 before upload. */
enum { HEGPU_BCAST_FLAT = 1, HEGPU_BCAST_TREE = 2, HEGPU_BCAST_STAGED = 0x100, HEGPU_BCAST_SAME_DEVICE = 0x200 };
int hegpu_context_clone(const hegpu_context* src, hegpu_context** out);
int hegpu_context_upload_device(hegpu_context* ctx, int device);
int hegpu_context_device(const hegpu_context* ctx);
int hegpu_broadcast_key(hegpu_context* const* ctxs, int n_ctx, uint64_t* const* keys, size_t elems,
                        const hegpu_stream* streams);
int hegpu_broadcast_bytes(const int* devices, int n, void* const* bufs, size_t bytes, const hegpu_stream* streams,
                          int* path_out);
int hegpu_last_broadcast_path(void);
/* integer properties: "n_power","Q_size","P_size","Q_prime_size","bsk_modulus" */
long hegpu_context_int(const hegpu_context* ctx, const char* name);
/* copy the named HOST table (reference member name without trailing '_',
 * e.g. "modulus","ntt_table","last_q_modinv","base_change_matrix_Bsk")
 * into out[cap]; returns the element count, <0 if unknown / too small */
long hegpu_context_get(const hegpu_context* ctx, const char* name, uint64_t* out, long cap);
/* device address of a named device table ("new_prime_locations", ...) */
const void* hegpu_context_device_ptr(const hegpu_context* ctx, const char* name);
/* keygeneration.cu:684-728 steps_to_galois_elt; 0 for |steps| >= N/2 (the reference prints an error and
 * returns 0 there); -1 only if the host code failed (no exception crosses this boundary) */
int hegpu_steps_to_galois_elt(int steps, int coeff_count, int group_order);

/* ------------------------------------------------------------------ NTT seam
 * gpuntt::GPU_NTT / GPU_NTT_Inplace / GPU_INTT / GPU_INTT_Inplace
 *   (call sites src/lib/host/bfv/operator.cu:393,410; ckks/operator.cu:919,1011)
 * gpuntt::GPU_NTT_Modulus_Ordered_Inplace  (ckks/operator.cu:956,1524)
 * gpuntt::GPU_NTT_Poly_Ordered_Inplace     (ckks/operator.cu:996,1197)
 * `batch` polynomials of N coefficients; polynomial i uses modulus
 * mod_offset + (mod_order ? mod_order[i % mod_count] : i % mod_count) of the
 * chosen table set and lives at slot (poly_order ? poly_order[i] : i).
 * mod_order / poly_order are DEVICE int arrays or NULL.  in == out allowed. */
int hegpu_ntt(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int inverse, int batch,
              int mod_count, int mod_offset, const int* mod_order, const int* poly_order, hegpu_stream stream);

/* The six gpuntt:: entry points by name, for a maintainer who binds call site by call site.  The
 * reference passes table / modulus / n^-1 pointers (offset by the caller for a sub-chain) and an
 * ntt_rns_configuration; here the context owns the tables, so `table_set` + `mod_offset` select what those
 * pointers selected, `inverse` is cfg.ntt_type == INVERSE (n^-1 of the same moduli is applied, as
 * cfg.mod_inverse does), cfg.stream is the last argument.  All return 0 or an error code.
 *   gpuntt::GPU_NTT(in, out, tables, moduli, cfg, batch, mod_count)              bfv/operator.cu:393
 *   gpuntt::GPU_NTT_Inplace(inout, tables, moduli, cfg, batch, mod_count)        ckks/operator.cu:1011
 *   gpuntt::GPU_INTT(in, out, itables, moduli, cfg, batch, mod_count)            ckks/operator.cu:1461
 *   gpuntt::GPU_INTT_Inplace(inout, itables, moduli, cfg, batch, mod_count)      bfv/operator.cu:410, ckks :919
 *   gpuntt::GPU_NTT_Modulus_Ordered_Inplace(inout, tables, moduli, cfg, batch, mod_count, order)   ckks :956,1524
 *   gpuntt::GPU_NTT_Poly_Ordered_Inplace(inout, tables, moduli, cfg, batch, mod_count, order)      ckks :996,1197
 * `order` is a DEVICE int array, as in the reference. */
int hegpu_GPU_NTT(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int mod_offset, int batch,
                  int mod_count, hegpu_stream stream);
int hegpu_GPU_NTT_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int mod_offset, int batch,
                          int mod_count, hegpu_stream stream);
int hegpu_GPU_INTT(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int mod_offset, int batch,
                   int mod_count, hegpu_stream stream);
int hegpu_GPU_INTT_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int mod_offset, int batch,
                           int mod_count, hegpu_stream stream);
int hegpu_GPU_NTT_Modulus_Ordered_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int inverse,
                                          int mod_offset, int batch, int mod_count, const int* order,
                                          hegpu_stream stream);
int hegpu_GPU_NTT_Poly_Ordered_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int inverse,
                                       int mod_offset, int batch, int mod_count, const int* order,
                                       hegpu_stream stream);

/* ------------------------------------------------------------------ kernels
 * 1:1 replacements of the reference __global__ kernels (grid dims become
 * arguments).  `table_set` selects the modulus array (Q' chain or q|Bsk). */
/* src/lib/kernel/addition.cu:10-47 ; op 0=addition 1=substraction 2=negation */
int hegpu_addition(hegpu_context* ctx, const uint64_t* in1, const uint64_t* in2, uint64_t* out, int limbs,
                   int parts, int batch, int op, hegpu_stream stream);
/* src/lib/kernel/multiplication.cu:102-126 */
int hegpu_cross_multiplication(hegpu_context* ctx, int table_set, const uint64_t* in1, uint64_t in1_stride,
                               const uint64_t* in2, uint64_t in2_stride, uint64_t* out, uint64_t out_stride,
                               int decomp_size, int batch, hegpu_stream stream);
/* src/lib/kernel/switchkey.cu:11-59,1558-1619: out[d][i][n] = in[d][n] mod
 * q_{i < split ? i : i+level} for d < digits, i < nmods */
int hegpu_cipher_broadcast(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                           uint64_t out_stride, int digits, int nmods, int split, int level, int batch,
                           hegpu_stream stream);
/* mod_raise_kernel (src/lib/kernel/bootstrapping.cu:339-376; restated, not compiled against): the q_0 limb of each part,
 * coefficient domain, lifted to its centred representative c (v >= q_0 >> 1: c = v - q_0) and written into q_0 ..
 * q_{limbs-1}.  in [parts][1][N], out [parts][limbs][N] per item; limb 0 is the input word, limb j > 0 is |c| mod q_j for
 * c >= 0 and q_j - (|c| mod q_j) for c < 0 -- the word q_j itself when q_j divides |c|, as the reference writes it.
 * HEGPU_E_INVALID, out untouched: a NULL pointer, batch < 1 or > 65535, parts outside [1, 3], limbs outside [1, Q], out
 * overlapping in. */
int hegpu_mod_raise(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out, uint64_t out_stride,
                    int limbs, int parts, int batch, hegpu_stream stream);
/* src/lib/kernel/switchkey.cu:61-398: out[c][y][n] = sum_i in[i][y][n] * key[i][c][kidx(y)][n],
 * kidx(y) = y < split ? y : y + level (non-leveled: split = nmods, level = 0;
 * method I leveled: split = l, level = depth; method II leveled: same) */
int hegpu_keyswitch_multiply_accumulate(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride,
                                        const uint64_t* key, uint64_t* out, uint64_t out_stride, int digits,
                                        int nmods, int key_limbs, int split, int level, int batch,
                                        hegpu_stream stream);
/* src/lib/kernel/switchkey.cu:872-927,985-1046 (method II digit -> Q~ base conversion, P_size > 1) */
int hegpu_base_conversion_DtoQtilde(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                                    uint64_t out_stride, int depth, int batch, hegpu_stream stream);
/* src/lib/kernel/switchkey.cu:400-478 */
int hegpu_divide_round_lastq(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                             uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int switchkey, int batch,
                             hegpu_stream stream);
/* src/lib/kernel/switchkey.cu:1621-1813 (scheme of ctx picks bfv/ckks form) */
int hegpu_divide_round_lastq_permute(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride,
                                     const uint64_t* in2, uint64_t in2_stride, uint64_t* out,
                                     uint64_t out_stride, int galois_elt, int depth, int batch,
                                     hegpu_stream stream);
/* ---- the leveled (CKKS) mod-down, rescale and multi-prime mod-down kernels, launch by launch.  l = Q - depth is the
 * reference's current_decomp_count; every layout is [2][limbs][N] per item.
 * divide_round_lastq_leveled_stage_one_kernel (switchkey.cu:678-705): the last limb of each part of `in`, + half,
 * reduced into every kept modulus, - half_mod.
 *   rescale == 0 (relinearize / rotate, ckks/operator.cu:1003): in [2][l+1][N] with the special-prime limb at slot l,
 *                out [2][l][N], tables half / half_mod;
 *   rescale != 0 (rescale, ckks/operator.cu:1205): in [2][l][N] with q_{l-1} at slot l-1, out [2][l-1][N], tables
 *                rescaled_half + depth / rescaled_half_mod + location(depth). */
int hegpu_divide_round_lastq_leveled_stage_one(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                                               uint64_t out_stride, int rescale, int depth, int batch,
                                               hegpu_stream stream);
/* divide_round_lastq_leveled_stage_two_kernel / _switchkey_kernel (switchkey.cu:707-771): out = (in - in_last) *
 * P^-1 + ct over [2][l][N]; in_last [2][l][N] (the NTT of stage one's output), in [2][l+1][N]; switchkey != 0 adds
 * ct to part 0 only.  ct may alias out. */
int hegpu_divide_round_lastq_leveled_stage_two(hegpu_context* ctx, const uint64_t* in_last, uint64_t last_stride,
                                               const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                                               uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int switchkey,
                                               int depth, int batch, hegpu_stream stream);
/* move_cipher_leveled_kernel (switchkey.cu:776-790, ckks/operator.cu:1219): the l-1 kept limbs of both parts,
 * [2][l][N] -> [2][l][N] (part stride l on both sides) */
int hegpu_move_cipher_leveled(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                              uint64_t out_stride, int depth, int batch, hegpu_stream stream);
/* divide_round_lastq_rescale_kernel (switchkey.cu:792-815, ckks/operator.cu:1225): out [2][l-1][N] =
 * (in - in_last) * q_{l-1}^-1; in_last [2][l-1][N], in [2][l][N]; tables rescaled_last_q_modinv + location(depth) */
int hegpu_divide_round_lastq_rescale(hegpu_context* ctx, const uint64_t* in_last, uint64_t last_stride,
                                     const uint64_t* in, uint64_t in_stride, uint64_t* out, uint64_t out_stride,
                                     int depth, int batch, hegpu_stream stream);
/* divide_round_lastq_extended_kernel (switchkey.cu:480-543: + ct on both parts, BFV method II relinearize),
 * _extended_switchkey_kernel (:545-611: + ct on part 0) and _extended_leveled_kernel (:1222-1282: no ct, CKKS
 * method II): mod-down by the P_size special primes, one after the other.  in [2][rc][N] (rc = Q' - depth,
 * coefficient domain), out / ct [2][l][N].  mode 0 leveled (ct ignored), 1 ct on both parts, 2 ct on part 0. */
int hegpu_divide_round_lastq_extended(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                                      uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int mode, int depth,
                                      int batch, hegpu_stream stream);
/* src/lib/kernel/multiplication.cu:10-100 / 128-272 (BFV BEHZ) */
int hegpu_fast_convertion(hegpu_context* ctx, const uint64_t* in1, uint64_t in1_stride, const uint64_t* in2,
                          uint64_t in2_stride, uint64_t* out, uint64_t out_stride, int batch,
                          hegpu_stream stream);
int hegpu_fast_floor(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                     uint64_t out_stride, int batch, hegpu_stream stream);

/* ------------------------------------------------------------------ operators
 * HEArithmeticOperator<S> sequences, batched over independent ciphertexts.
 * `ws` is a caller-provided device workspace of at least
 * hegpu_workspace_bytes(ctx, op, depth, batch) bytes.
 *
 * Streams and capture.  Every entry of this header with a `stream` argument
 * issues all its work on that stream, and only there; it allocates nothing
 * and takes its temporaries from `ws`.  Host arrays (keys, elements, index
 * tables, plans) are read before the call returns.
 * Every such entry may be recorded into a hipGraph and replayed, on a context
 * that is uploaded and after one call outside the capture (module loading),
 * except two groups:
 *   - the entries that draw randomness: every entry that takes a hegpu_rng*
 *     (hegpu_generate_*, hegpu_*_encrypt, the hegpu_mpc_*_share entries,
 *     hegpu_tfhe_generate_* and hegpu_tfhe_encrypt).  The generator's
 *     counter advances on the host at the call: a replay would draw the same
 *     a, noise and u again, and two encryptions with the same randomness leak
 *     the difference of their messages;
 *   - the entries that synchronise: hegpu_generate_secret_key,
 *     hegpu_tfhe_prepare_bootkey, hegpu_tfhe_status and
 *     hegpu_tfhe_prepared_format.
 * On a stream that is being captured these return HEGPU_E_LOGIC (the message
 * says "draws randomness" or "synchronises") before anything is queued and
 * before the generator's counter moves; the capture stays valid.
 * hegpu_tfhe_prepared_format takes no stream and cannot ask: called during a
 * capture it returns -1 and the capture is lost.
 * hegpu_mpc_ckks_refresh_merge / hegpu_mpc_bfv_refresh_merge take the common
 * generator only to derive the public `a` of the shares again; they draw
 * nothing of their own and are capturable.  A replay derives the `a` of the
 * captured call, so the shares of every replay must come from a common
 * generator as far advanced as the one the capture was given. */
enum {
    HEGPU_OP_CKKS_RELIN = 1,
    HEGPU_OP_CKKS_RESCALE = 2,
    HEGPU_OP_CKKS_GALOIS = 3,
    HEGPU_OP_BFV_MULTIPLY = 4,
    HEGPU_OP_BFV_RELIN = 5,
    HEGPU_OP_BFV_GALOIS = 6,
    HEGPU_OP_KEYGEN_SECRET = 7,
    HEGPU_OP_KEYGEN_PUBLIC = 8,
    HEGPU_OP_KEYGEN_SWITCH = 9, /* relinearisation and Galois keys */
    HEGPU_OP_CKKS_ENCRYPT = 10,
    HEGPU_OP_BFV_ENCRYPT = 11,
    HEGPU_OP_BFV_DECRYPT = 12,
    HEGPU_OP_BFV_DECODE = 13,
    HEGPU_OP_CKKS_ENCODE = 14,
    HEGPU_OP_CKKS_DECODE = 15, /* depth-dependent */
    HEGPU_OP_BFV_MULTIPLY_PLAIN = 16,
    HEGPU_OP_CKKS_ROTATE_HOISTED = 17, /* hegpu_ckks_rotate_hoisted with room for four accumulators */
    HEGPU_OP_MPC_KEY_SHARE = 18,        /* every hegpu_mpc_*_key_share* entry */
    HEGPU_OP_MPC_BFV_DECRYPT_MERGE = 19, /* per ciphertext of the batch */
    HEGPU_OP_MPC_REFRESH_SHARE = 20,     /* hegpu_mpc_*_refresh_share: 0 bytes, the share is built in place */
    HEGPU_OP_MPC_REFRESH_MERGE = 21,     /* hegpu_mpc_*_refresh_merge; per item: CKKS (Q - depth) N words, BFV (Q + 1) N */
    HEGPU_OP_CKKS_LOGIC_GATE = 22,       /* hegpu_ckks_logic_gate: a three-part product per item + the larger of RELIN, RESCALE */
    HEGPU_OP_BFV_LOGIC_GATE = 23,        /* hegpu_bfv_logic_gate: the same + the largest of MULTIPLY, RELIN, MULTIPLY_PLAIN */
    /* 24 stays unassigned: tests/test_cabi_logic.py holds it as the number no row has (0 bytes) */
    HEGPU_OP_CKKS_MOD_RAISE = 25,        /* hegpu_ckks_mod_raise: 2 N words per item at every depth */
    HEGPU_OP_CKKS_BOOTSTRAP = 26         /* the head of hegpu_ckks_bootstrap's workspace, 6 N words per item at every depth; the
                                          * whole is hegpu_ckks_bootstrap_workspace_bytes */
};
size_t hegpu_workspace_bytes(const hegpu_context* ctx, int op, int depth, int batch);

/* HEOperator<CKKS>::multiply_ckks (src/lib/host/ckks/operator.cu:796-837):
 * ct [2][l][N] x [2][l][N] -> out [3][l][N], l = Q - depth */
int hegpu_ckks_multiply(hegpu_context* ctx, const uint64_t* ct1, uint64_t ct1_stride, const uint64_t* ct2,
                        uint64_t ct2_stride, uint64_t* out, uint64_t out_stride, int depth, int batch,
                        hegpu_stream stream);
/* relinearize_inplace (host/ckks/operator.cuh:1053-1094): key-switch method I
 * when P_size == 1 (relinearize_seal_method_inplace_ckks, ckks/operator.cu:899-1023,
 * relin_key [Q][2][Q'][N]), method II when P_size > 1
 * (relinearize_external_product_method2_inplace_ckks, ckks/operator.cu:1025-1154,
 * relin_key [d][2][Q'][N]).  ct [3][l][N] -> first two parts, in place. */
int hegpu_ckks_relinearize_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t ct_stride,
                                   const uint64_t* relin_key, int depth, int batch, void* ws, size_t ws_bytes,
                                   hegpu_stream stream);
/* The modulus raise of bootstrapping (mod_up_from_q0, ckks/operator.cu:3963-4033, without its two key switches): ct
 * [2][1][N] per item, a ciphertext at depth Q - 1 (NTT domain) -> out [2][Q - out_depth][N], NTT domain: every coefficient
 * of the q_0 limbs lifted as hegpu_mod_raise lifts it.  One inverse transform of the two limbs, one forward transform whose
 * first load is the lift, one copy of limb 0.  Canonical residues, bit-identical to hegpu_ntt (inverse) ->
 * hegpu_mod_raise -> hegpu_ntt (forward).  HEGPU_E_INVALID before anything is queued: a NULL pointer, batch < 1, out_depth
 * outside [0, Q - 1], a workspace below HEGPU_OP_CKKS_MOD_RAISE, out overlapping ct, the workspace overlapping either. */
int hegpu_ckks_mod_raise(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out, uint64_t out_stride,
                         int out_depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* rescale_inplace_ckks_leveled (ckks/operator.cu:1156-1244):
 * ct [2][l][N] -> [2][l-1][N] in place (caller then uses depth+1) */
int hegpu_ckks_rescale_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t ct_stride, int depth, int batch,
                               void* ws, size_t ws_bytes, hegpu_stream stream);
/* apply_galois_ckks_method_I (ckks/operator.cu:1422-1559); the result buffer must not contain the input: HEGPU_E_INVALID
 * if the address ranges of the two batches overlap (the epilogue scatters results while c0 is still being read) */
int hegpu_ckks_apply_galois(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out,
                            uint64_t out_stride, const uint64_t* galois_key, int galois_elt, int depth,
                            int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* fast_single_hoisting_rotation_ckks (host/ckks/operator.cuh:2133-2196; method I ckks/operator.cu:4674-4953,
 * method II :5092-5446): `count` Galois automorphisms of ONE ciphertext per batch item.  The INTT of the
 * ciphertext, the digit decomposition and the forward NTT of the digits do not depend on the element and run
 * once; per element: key inner product, INTT, mod-down + permutation, NTT.  Entry i is written to
 * out + i * 2 l N (per item: out_stride apart), l = Q - depth; galois_elts[i] == 0 copies the input (the
 * reference's result[0] / a zero shift).  galois_keys / galois_elts are HOST arrays of length count;
 * galois_keys[i] is the DEVICE key of element i (ignored for 0).  Every entry is bit-identical to
 * hegpu_ckks_apply_galois with the same element and key.  Workspace: HEGPU_OP_CKKS_GALOIS is enough; with
 * HEGPU_OP_CKKS_ROTATE_HOISTED (room for four accumulators) the inner products of four elements at a time share one
 * read of the digits. */
int hegpu_ckks_rotate_hoisted(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out,
                              uint64_t out_stride, const uint64_t* const* galois_keys, const int* galois_elts,
                              int count, int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* The inner sums of a baby-step/giant-step product of a plaintext matrix, given by its diagonals, with an encrypted
 * vector: cipherplain_multiply_accumulate_kernel (src/lib/kernel/multiplication.cu), which the reference launches once
 * per giant step (host/ckks/operator.cu:2843) -- here ONE launch computes all n2 sums: the n1 rotated ciphertexts are
 * read once, every diagonal once, the products of a sum are added as 128-bit integers and reduced once.
 *   out entry j [p] = sum_i diags[index[j][i]] (.) rot entry i [p]   mod q_limb,   p = 0, 1
 * rot: n1 ciphertexts per item in the layout hegpu_ckks_rotate_hoisted writes (entry i at rot + i * 2 l N, items
 * rot_stride apart), l = Q - depth; diags: DEVICE [n_diag][l][N] plaintext limbs (NTT domain, shared by the items);
 * index: HOST [n2][n1], -1 = absent (a row of -1 gives zeros); out entry j at out + j * 2 l N, items out_stride apart.
 * Every result is bit-identical to hegpu_cipherplain_multiplication + hegpu_addition per diagonal.
 * HEGPU_E_INVALID: n1 or n2 outside [1, 16] (16 products of residues below 2^60 fit the 128-bit sum; the index table
 * travels by value), an index >= n_diag or < -1, out overlapping rot. */
int hegpu_ckks_diag_mac(hegpu_context* ctx, const uint64_t* rot, uint64_t rot_stride, int n1, const uint64_t* diags,
                        int n_diag, const int* index, int n2, uint64_t* out, uint64_t out_stride, int depth, int batch,
                        hegpu_stream stream);
/* y = M v for a plaintext matrix M and an encrypted vector v (this backend's own entry: the reference's
 * multiply_matrix, host/ckks/operator.cu:2803-2895, is private to its bootstrapping):
 *   out = sum_j galois(giant_elts[j], sum_i diags[index[j][i]] (.) galois(baby_elts[i], ct))
 * as hegpu_ckks_rotate_hoisted of the n1 baby steps, one hegpu_ckks_diag_mac, one hegpu_ckks_apply_galois per giant
 * step with a non-zero element, and one sum of the n2 terms.  Element 0 = no rotation (its key is ignored); keys and
 * elements are HOST arrays of DEVICE keys, [n1] and [n2].  The result has two parts at the same depth and is NOT
 * rescaled: its scale is the product of the ciphertext's and the diagonals' scales.  Bit-identical to the same
 * composition of the single entries.  out must not overlap ct.  Workspace: the size function below (it depends on n1
 * and n2, so it is not a row of hegpu_workspace_bytes). */
size_t hegpu_ckks_linear_transform_workspace_bytes(const hegpu_context* ctx, int n1, int n2, int depth, int batch);
int hegpu_ckks_linear_transform(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out,
                                uint64_t out_stride, const uint64_t* diags, int n_diag, const int* index, int n1, int n2,
                                const uint64_t* const* baby_keys, const int* baby_elts,
                                const uint64_t* const* giant_keys, const int* giant_elts, int depth, int batch, void* ws,
                                size_t ws_bytes, hegpu_stream stream);
/* Chained giant steps: the same product over a reduced set of Galois keys (this backend's own schedule; the reference's
 * less_key_mode, multiply_matrix_less_memory, host/ckks/operator.cu:3399-3496, rotates inner sum j by the first giant
 * step j times, O(n2^2) key switches -- this one keeps the n2 - 1 of the direct mode).
 *
 * hegpu_giant_step_chain (HOST ONLY, no context, no device): the Horner fold over a plan's giant shifts.  Each shift in
 * [0, slots) is taken as its signed representative in (-slots/2, slots/2].  The non-negative shifts, ascending, each have
 * the one before as parent; the negative ones, from the one nearest zero outwards, likewise, the first of them hanging on
 * the zero shift if there is one.  parent[j] = -1: a root.  link_shifts[j] in [0, slots): term j's signed shift minus its
 * parent's, for a root its own shift.  The links a term crosses add up to its shift modulo slots, so the plan's
 * pre-rotated diagonals stay as they are; giant steps that are dense on both sides of zero need two distinct links.
 * HEGPU_E_INVALID: n2 outside [1, 16], slots no power of two, a shift outside [0, slots), a null argument.
 *
 * hegpu_ckks_linear_transform_chained: hegpu_ckks_linear_transform with giant_parent, a HOST array [n2].  NULL, or all
 * -1, is hegpu_ckks_linear_transform itself (which is this entry with NULL).  Otherwise giant_elts[j] / giant_keys[j]
 * describe term j's LINK (element 0 = no rotation, its key is ignored) and
 *   S_j = inner_j + sum over the children k of j of galois(giant_elts[k], S_k)
 *   out = sum over the roots r of galois(giant_elts[r], S_r)
 * evaluated deepest terms first: one hegpu_ckks_apply_galois per link with a non-zero element, one sum per term with
 * children, one over the roots if there are several.  Bit-identical to the same composition of the single entries
 * (hegpu_ckks_rotate_hoisted, hegpu_cipherplain_multiplication + hegpu_addition per diagonal, hegpu_ckks_apply_galois per
 * link, hegpu_addition).  The workspace is hegpu_ckks_linear_transform_workspace_bytes in both modes.
 * HEGPU_E_INVALID, nothing launched: what hegpu_ckks_linear_transform refuses, a parent outside [-1, n2), a term that is
 * its own ancestor, a non-zero link element with a null key. */
int hegpu_giant_step_chain(const int* giant_shifts, int n2, int slots, int* parent, int* link_shifts);
int hegpu_ckks_linear_transform_chained(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out,
                                        uint64_t out_stride, const uint64_t* diags, int n_diag, const int* index, int n1,
                                        int n2, const uint64_t* const* baby_keys, const int* baby_elts,
                                        const uint64_t* const* giant_keys, const int* giant_elts, const int* giant_parent,
                                        int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* ---- CoeffToSlot / SlotToCoeff (HEArithmeticOperator<CKKS>::coeff_to_slot / slot_to_coeff, host/ckks/operator.cu:
 * 3566-3663 and 3809-3891; the context of generate_encoding_transform_context, :6686-6800).
 *
 * With n = N/2, L = log2 n and zeta = exp(2 pi i / 2N), the slot vector of a polynomial with real coefficients a is
 * z = U w, w_k = a_k + i a_{k+n}, U[j][k] = zeta^(5^j k) = F_L ... F_1 B: the radix-2 stages of the encoder's special
 * FFT and the bit reversal B on L bits.  Neither transform applies B: CoeffToSlot leaves slot j holding coefficient
 * bitrev_L(j) (out0) and n + bitrev_L(j) (out1), SlotToCoeff expects them so.
 *
 * hegpu_encoding_transform_shape / _fill (HOST ONLY, no device needed): the L stages in `pieces` in [2, 5] groups of
 * floor(L / pieces) or ceil(L / pieces) consecutive stages, the larger groups first, in the order they are applied.
 * inverse = 0 (SlotToCoeff): group 0 holds stage 1.  inverse = 1 (CoeffToSlot): group 0 holds stage L, every stage is
 * inverted, and each group carries the factor 2^(-1/pieces), so that all groups together are 1/2 B U^-1.
 * _shape writes, per group: the stride 2^s (every diagonal offset of the group is a multiple of it), the number of
 * stages g and the number of non-zero diagonals (at most 2^(g+1) - 1).  _fill writes one group: its signed offsets in
 * (-n/2, n/2], ascending, and values [n_diag][n] (re, im) pairs with diag_k[t] = M[t][(t + k) mod n].
 * HEGPU_E_INVALID: a degree that is no power of two, pieces outside [2, 5] or above L, a wrong piece or n_diag. */
int hegpu_encoding_transform_shape(int coeff_count, int inverse, int pieces, int* strides, int* stages, int* n_diags);
int hegpu_encoding_transform_fill(int coeff_count, int inverse, int pieces, int piece, int n_diag, int* offsets,
                                  double* values);
/* The two passes at the real / imaginary boundary, each one read of every input and one write of every output, both
 * parts, the Q - out_depth limbs that are kept (out_depth >= depth: the dropped limbs are neither read nor written):
 *   conj_split: out0 = x + xc, out1 = div_i(x - xc)     (xc = the conjugate of x: out0 = 2 Re, out1 = 2 Im)
 *   conj_merge: out = c0 + mult_i(c1)
 * Inputs [2][Q - depth][N], outputs [2][Q - out_depth][N] per item.  Bit-identical to hegpu_addition (op 0 / 1) and
 * hegpu_ckks_mult_i (divide = 1 / 0) on the kept limbs.  HEGPU_E_INVALID, outputs untouched: an output overlapping an
 * input (or the other output), out_depth < depth or >= Q, batch < 1. */
int hegpu_ckks_conj_split(hegpu_context* ctx, const uint64_t* x, uint64_t x_stride, const uint64_t* xc,
                          uint64_t xc_stride, uint64_t* out0, uint64_t* out1, uint64_t out_stride, int depth,
                          int out_depth, int batch, hegpu_stream stream);
int hegpu_ckks_conj_merge(hegpu_context* ctx, const uint64_t* c0, uint64_t c0_stride, const uint64_t* c1,
                          uint64_t c1_stride, uint64_t* out, uint64_t out_stride, int depth, int out_depth, int batch,
                          hegpu_stream stream);
/* One factor of a sequence: exactly the matrix arguments of hegpu_ckks_linear_transform_chained (all arrays HOST, keys
 * and diagonals DEVICE).  The diagonals of factor k are encoded at the depth the chain has reached: depth + k for
 * CoeffToSlot, depth + 1 + k for SlotToCoeff.  giant_parent: NULL (a zeroed field) = the direct mode, the arguments of
 * hegpu_ckks_linear_transform; otherwise the factor's giant steps are chained and giant_keys / giant_elts are its links. */
typedef struct hegpu_linear_factor {
    const uint64_t* diags;
    int n_diag;
    const int* index;
    int n1, n2;
    const uint64_t* const* baby_keys;
    const int* baby_elts;
    const uint64_t* const* giant_keys;
    const int* giant_elts;
    const int* giant_parent;
} hegpu_linear_factor;
/* coeff_to_slot: per factor hegpu_ckks_linear_transform + hegpu_ckks_rescale_inplace (depth -> depth + count), then
 * hegpu_ckks_apply_galois with the element 2N - 1 and conj_key, then hegpu_ckks_conj_split to depth + count + 1 -- the
 * depth at which the reference's outputs leave (it spends that level on a product with scale / 2; here the half is in
 * the matrices).  out0, out1: [2][Q - depth - count - 1][N] per item, out_stride apart.
 * slot_to_coeff: hegpu_ckks_conj_merge from depth to depth + 1 (the reference spends a level on its product with i),
 * then count x (linear transform, rescale).  The last product is written to out and rescaled there: out needs room for
 * [2][Q - depth - count][N] per item and holds [2][Q - depth - count - 1][N] on return.
 * Both are bit-identical to the same chain of single entries (a factor with giant_parent:
 * hegpu_ckks_linear_transform_chained, itself bit-identical to the same composition of single entries).  HEGPU_E_INVALID,
 * outputs untouched: count < 1, depth + count + 1 >= Q, an output overlapping an input, what
 * hegpu_ckks_linear_transform_chained refuses in a factor, a
 * workspace below hegpu_ckks_encoding_transform_workspace_bytes (0 for arguments it cannot size). */
size_t hegpu_ckks_encoding_transform_workspace_bytes(const hegpu_context* ctx, const hegpu_linear_factor* factors,
                                                     int count, int depth, int batch);
int hegpu_ckks_coeff_to_slot(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out0, uint64_t* out1,
                             uint64_t out_stride, const hegpu_linear_factor* factors, int count,
                             const uint64_t* conj_key, int depth, int batch, void* ws, size_t ws_bytes,
                             hegpu_stream stream);
int hegpu_ckks_slot_to_coeff(hegpu_context* ctx, const uint64_t* c0, uint64_t c0_stride, const uint64_t* c1,
                             uint64_t c1_stride, uint64_t* out, uint64_t out_stride, const hegpu_linear_factor* factors,
                             int count, int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* ------------------------------------------------------------------ polynomial evaluation on a CKKS ciphertext
 * (this backend's own entries: the reference's evaluate_poly, host/ckks/operator.cu:4292-4671, is protected and reachable
 * only through its bootstraps).  Three layers: a host-only plan, two one-pass kernels, one sequence that executes a plan.
 *
 * PLAN.  hegpu_poly_eval_plan_size / _fill are host only (no context, no device) and reproduce the reference's schedule:
 * baby powers 2^s - 1 .. 1 and giant powers 2^s .. 2^(D-1) with s = optimal_split(D), the recursion of
 * evaluate_poly_recurse with its lead_ / max_deg_ rules and split_coeffs, its target-scale bookkeeping and its two
 * conditional rescales.  basis: HEGPU_POLY_MONOMIAL or HEGPU_POLY_CHEBYSHEV (on [-1, 1]); coeffs: n_coeffs = degree + 1
 * (re, im) pairs c_0 .. c_d; max_deg / lead: Polynomial::max_deg_ / lead_ (max_deg = degree and lead = 1 for a polynomial
 * of its own); level / scale: of the input ciphertext (level = index of its last prime = Q - 1 - depth); primes: the
 * context's q_0 .. q_{n_primes - 1}.  D is the bit length of the degree (the reference's ceil(log2(degree)) but for a
 * power of two, where its first split reads a power it never made); the rescale of q compares with target_scale / 2.
 * The plan is a list of steps over numbered registers: register 0 is the input, step k writes register k + 1, the last
 * step's register is the result, at the level and scale that step carries.
 *   POWER    dst = reg[a] * reg[b] at mul_level (the lower of the two), relinearized, rescaled; then c = HEGPU_POLY_TAIL_NONE:
 *            nothing (monomial); HEGPU_POLY_TAIL_ONE: dst = 2 dst - round(tail_const); c >= 0: dst = 2 dst - reg[c]
 *   LEAF     dst = w0 + sum_i w[i] * reg[term_reg[i]] over level + 1 limbs; w[i] = round(c_i * (leaf_scale / scale_i)),
 *            w0 = round(c_0 * leaf_scale), real and imaginary part separately; terms with w[i] == 0 are left out
 *   COMBINE  dst = reg[a] * reg[b] + reg[c]: reg[a] rescaled first if rescale_first, product at mul_level, relinearized,
 *            sum at the lower of mul_level and reg[c]'s level; rescale_after: the sum is rescaled (the planner sets it on
 *            the polynomial's last step; an EvalMod plan goes on from there)
 * HEGPU_E_INVALID, outputs untouched: degree < 2, a leaf of more than 15 power terms (degree > 255), too few levels for
 * the polynomial's depth, a non-finite coefficient or scale, max_deg < degree, n_steps not what _size gives. */
enum { HEGPU_POLY_MONOMIAL = 0, HEGPU_POLY_CHEBYSHEV = 1 };
enum { HEGPU_POLY_POWER = 0, HEGPU_POLY_LEAF = 1, HEGPU_POLY_COMBINE = 2 };
enum { HEGPU_POLY_TAIL_NONE = -1, HEGPU_POLY_TAIL_ONE = -2 };
typedef struct hegpu_poly_step {
    /* kind: HEGPU_POLY_POWER / _LEAF / _COMBINE; dst: the register written (= 1 + the step's position);
     * a, b: POWER: dst = reg[a] * reg[b]; COMBINE: dst = reg[a] * reg[b] + reg[c] (a = q, b = the giant power);
     * c: POWER: HEGPU_POLY_TAIL_NONE (monomial), HEGPU_POLY_TAIL_ONE (2 dst - 1) or the register of 2 dst - reg[c]; COMBINE: r */
    int32_t kind, dst, a, b, c;
    int32_t level;         /* of dst */
    int32_t mul_level;     /* POWER, COMBINE: the level of the product (the lower of its operands', after q's rescale) */
    int32_t rescale_first; /* COMBINE: 1 = reg[a] is rescaled before the product */
    int32_t rescale_after; /* the polynomial's last step only: 1 = dst is rescaled once more; level and scale are those after it */
    int32_t n_terms;       /* LEAF: number of power terms, <= 15 */
    int32_t term_reg[15];
    double scale;          /* of dst */
    double tail_const;     /* POWER with HEGPU_POLY_TAIL_ONE: the real constant subtracted from part 0 (= scale: the one) */
    double w0[2];          /* LEAF: round(c_0 * leaf_scale), (re, im) */
    double w[15][2];       /* LEAF: round(c_i * (leaf_scale / scale_i)) per term */
} hegpu_poly_step;
int hegpu_poly_eval_plan_size(int basis, const double* coeffs, int n_coeffs, int max_deg, int lead, int level, double scale,
                              double target_scale, const uint64_t* primes, int n_primes, int* n_steps);
int hegpu_poly_eval_plan_fill(int basis, const double* coeffs, int n_coeffs, int max_deg, int lead, int level, double scale,
                              double target_scale, const uint64_t* primes, int n_primes, hegpu_poly_step* steps, int n_steps);
/* EVALMOD of CKKS bootstrapping (eval_mod, host/ckks/operator.cu:4248-4290) as a plan for the same sequence; host only.
 * The input holds u in [-1, 1] with K u = I + eps, I an integer, |I| < K.  With c = (1 / 2 pi)^(1 / 2^r), r = double_angle,
 * the plan is the Chebyshev plan of p, the degree-`degree` interpolant (at the Chebyshev nodes, in doubles) of
 * g(u) = c cos(2 pi (K u - 1/4) / 2^r), followed by r POWER steps y <- 2 y^2 - c^(2^(i+1)) (a = b = the previous register,
 * HEGPU_POLY_TAIL_ONE, tail_const = c^(2^(i+1)) at the step's scale): the result is sin(2 pi eps) / 2 pi at target_scale
 * (to the rounding of doubles), bit_length(degree) + r levels below `level`.  p carries the target scale of the reference's
 * square-root chain (:4257-4265); its change of variable (:4267-4271) is inside g, its q_diff corrections have no
 * counterpart (scales are exact labels here).  HEGPU_E_INVALID, outputs untouched: K < 1, double_angle outside [0, 8], a
 * degree hegpu_poly_eval_plan_* refuses, too few levels, a scale that is not positive and finite, n_steps not what _size
 * gives. */
int hegpu_eval_mod_plan_size(int K, int degree, int double_angle, int level, double scale, double target_scale,
                             const uint64_t* primes, int n_primes, int* n_steps);
int hegpu_eval_mod_plan_fill(int K, int degree, int double_angle, int level, double scale, double target_scale,
                             const uint64_t* primes, int n_primes, hegpu_poly_step* steps, int n_steps);
/* KERNELS.  weighted_sum: out[p] = (p == 0 ? w0 : 0) + sum_k w_k * terms[k][p] mod q_j over the first `limbs` limbs, p = 0, 1.
 * terms / term_strides / term_limbs / weights are HOST arrays of count <= 15 entries: term k is a DEVICE ciphertext
 * [2][term_limbs[k]][N] per item (term_limbs[k] >= limbs; read in place, its part 1 term_limbs[k] * N words after part 0),
 * items term_strides[k] apart; weights: (re, im) pairs of finite doubles, the Gaussian integer round(re) + round(im) i in
 * every slot.  15 products of residues below 2^61 and a residue fit the 128-bit sum that is reduced once.  Bit-identical to
 * hegpu_ckks_gaussian_integer_op (multiply) per term + hegpu_addition + hegpu_ckks_gaussian_integer_op (add) for w0.
 * double_sub: out = 2 a - b over the first `limbs` limbs of both parts; b == NULL: round(value) is subtracted from part 0
 * instead (|value| < 3.4e38).  a / b: [2][a_limbs / b_limbs][N] per item, both >= limbs.  Bit-identical to
 * hegpu_addition(a, a) + hegpu_addition (op 1) resp. hegpu_ckks_constant_op (HEGPU_CONST_SUB).
 * HEGPU_E_INVALID, out untouched: count outside [0, 15], a limb count outside [limbs, Q], a non-finite weight, batch < 1,
 * out overlapping a term or b; out overlapping a unless it is a itself with a_limbs == limbs (in place). */
int hegpu_ckks_weighted_sum(hegpu_context* ctx, const uint64_t* const* terms, const uint64_t* term_strides,
                            const int* term_limbs, const double* weights, int count, double w0_re, double w0_im,
                            uint64_t* out, uint64_t out_stride, int limbs, int batch, hegpu_stream stream);
int hegpu_ckks_double_sub(hegpu_context* ctx, const uint64_t* a, uint64_t a_stride, int a_limbs, const uint64_t* b,
                          uint64_t b_stride, int b_limbs, double value, uint64_t* out, uint64_t out_stride, int limbs,
                          int batch, hegpu_stream stream);
/* SEQUENCE.  Executes a plan on ct ([2][Q - depth][N] per item, the plan's input level = Q - 1 - depth) and nothing else:
 * POWER = hegpu_ckks_multiply + _relinearize_inplace + _rescale_inplace + one double_sub; LEAF = one weighted_sum;
 * COMBINE = the rescale, multiply, relinearize + one sum at the lower level.  An operand above the level of a product or
 * sum is copied down first.  One polynomial and one level serve the whole batch.  out receives the last step's register:
 * it needs room for [2][level + 1 + rescale_after][N] per item and holds [2][level + 1][N] on return, at the depth
 * Q - 1 - level and the scale of the plan's last step.  Bit-identical to the same plan executed with the single entries.
 * HEGPU_E_INVALID before anything is queued: a workspace below hegpu_ckks_poly_eval_workspace_bytes (0 for a plan it cannot
 * size), out overlapping ct, a register or level number out of range, more than 4096 steps, a tail constant that is not
 * finite or not below 3.4e38, a non-finite weight, null pointers, batch < 1, a plan that ends with a POWER step without a
 * tail (its register is three parts wide; one with a tail, as an EvalMod plan ends, writes out). */
size_t hegpu_ckks_poly_eval_workspace_bytes(const hegpu_context* ctx, const hegpu_poly_step* plan, int n_steps, int depth,
                                            int batch);
int hegpu_ckks_poly_eval(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out, uint64_t out_stride,
                         const hegpu_poly_step* plan, int n_steps, const uint64_t* relin_key, int depth, int batch,
                         void* ws, size_t ws_bytes, hegpu_stream stream);
/* ------------------------------------------------------------------ the CKKS refresh (regular_bootstrapping_v2,
 * generate_bootstrapping_params_v2 and mod_up_from_q0 with its two key switches, host/ckks/operator.cu:7147-7224, :6906-7000,
 * :3963-4033): a host-only plan that holds every scale label, and one sequence over the entries above.
 *
 * PLAN.  hegpu_bootstrap_plan_fill is host only.  config: the fields of the reference's EvalModConfig / EncodingMatrixConfig
 * with their defaults (ratio 256, K 16, degree 30, double_angle 3); levels are indices of a ciphertext's last prime;
 * eval_level / stc_level may be -1 (they follow from cts_level: eval_level = cts_level - cts_pieces - 1, stc_level =
 * eval_level - bit_length(sine_degree) - double_angle) and are refused if they are anything else.  With D = scale:
 *   k1 = max(1, round(q_0 / (ratio D))), D' = k1 D: the q_0 limbs are multiplied by k1 before the raise;
 *   the raised ciphertext is labelled raise_scale = q_0 K, its value is (I + eps) / K, eps = D' a / q_0;
 *   factor f of CoeffToSlot is encoded at cts_scale[f] (level cts_level - f) and leaves the label cts_label[f]; the last
 *   one is the sine scale q_(eval_level) to the rounding of doubles and the input scale eval_in_scale of the EvalMod plan
 *   hegpu_eval_mod_plan_*(K, sine_degree, double_angle, eval_level, eval_in_scale, eval_target_scale), whose result
 *   sin(2 pi eps) / 2 pi at eval_out_scale is relabelled stc_in_scale = eval_out_scale D' / q_0: the value is then
 *   f(a) = (rho / 2 pi) sin(2 pi a / rho), rho = q_0 / D'; factor g of SlotToCoeff is encoded at stc_scale[g] (level
 *   stc_level - 1 - g); the result is at out_level with the label out_scale = D to the rounding of doubles.
 * HEGPU_E_INVALID, *plan untouched: fewer levels than cts_pieces + 1 + bit_length(sine_degree) + double_angle + 1 +
 * stc_pieces and one limb left, K < 1, ratio D > q_0, a scale or ratio that is not positive and finite, piece counts
 * outside [2, 5], start levels that do not follow from one another, what hegpu_eval_mod_plan_* refuses. */
typedef struct hegpu_bootstrap_config {
    /* scale: D, the caller's scale; message_ratio: q_0 / D' aimed at (EvalModConfig::message_ratio_, default 256) */
    double scale, message_ratio;
    /* K: the raise's overflow I stays below K in magnitude (EvalModConfig::K_, default 16); sine_degree: EvalModConfig::sine_deg_,
     * default 30; double_angle: EvalModConfig::double_angle_, default 3 */
    int32_t K, sine_degree, double_angle;
    /* cts_level: EncodingMatrixConfig::level_start_ of CoeffToSlot, the level the raise goes to; eval_level:
     * EvalModConfig::level_start_; stc_level: EncodingMatrixConfig::level_start_ of SlotToCoeff (the merge drops to stc_level - 1) */
    int32_t cts_level, cts_pieces, eval_level, stc_level, stc_pieces;
} hegpu_bootstrap_config;
typedef struct hegpu_bootstrap_plan {
    uint64_t k1;
    int32_t cts_level, cts_pieces, eval_level, stc_level, stc_pieces, out_level;
    int32_t K, sine_degree, double_angle;
    int32_t reserved;
    double raise_scale; /* q_0 K */
    /* cts_scale[f]: the scale factor f's diagonals are encoded at (level cts_level - f); cts_label[f]: the ciphertext's label
     * after factor f and its rescale.  The factorisation of the special FFT has 2 .. 5 pieces. */
    double cts_scale[5], cts_label[5];
    double eval_in_scale, eval_target_scale, eval_out_scale;
    double stc_in_scale; /* the relabelled result of EvalMod */
    double stc_scale[5], stc_label[5]; /* factor g's diagonals (level stc_level - 1 - g) and the label after it */
    double out_scale; /* D to the rounding of doubles */
} hegpu_bootstrap_plan;
int hegpu_bootstrap_plan_fill(const hegpu_bootstrap_config* config, const uint64_t* primes, int n_primes,
                              hegpu_bootstrap_plan* plan);
/* SEQUENCE.  ct: [2][1][N] per item, a ciphertext at depth Q - 1 (what hegpu_ckks_mod_raise takes).  The launches, all on
 * `stream`, nothing allocated: the q_0 limbs times k1 (k1 > 1 only; without switch keys in the place of the raise's copy of
 * limb 0) -> with switch keys hegpu_ckks_apply_galois with the element 1 and swk_dense_to_sparse at depth Q - 1 ->
 * hegpu_ckks_mod_raise to plan->cts_level -> with switch keys the same key switch with swk_sparse_to_dense there ->
 * hegpu_ckks_coeff_to_slot (cts: cts_count = plan->cts_pieces factors) -> ONE hegpu_ckks_poly_eval of eval_mod over the
 * 2 * batch halves -> hegpu_ckks_slot_to_coeff (stc: stc_count = plan->stc_pieces factors).  Bit-identical to that chain of single entries
 * (the multiplication: hegpu_ckks_constant_op, HEGPU_CONST_MUL; a factor with giant_parent:
 * hegpu_ckks_linear_transform_chained, bit-identical to the same composition of single entries).  out needs room for [2][out_level + 2][N] per item and
 * holds [2][out_level + 1][N] on return, at depth Q - 1 - out_level and scale plan->out_scale.
 * HEGPU_E_INVALID before anything is queued, out untouched: exactly one of the two switch keys, a plan, EvalMod plan or
 * factor list that does not fit the context or one another, a workspace below hegpu_ckks_bootstrap_workspace_bytes (0 for
 * arguments it cannot size; switch_keys: whether the call passes them), out overlapping ct or the workspace, null
 * pointers, batch < 1. */
size_t hegpu_ckks_bootstrap_workspace_bytes(const hegpu_context* ctx, const hegpu_bootstrap_plan* plan,
                                            const hegpu_poly_step* eval_mod, int n_steps, const hegpu_linear_factor* cts,
                                            int cts_count, const hegpu_linear_factor* stc, int stc_count, int switch_keys,
                                            int batch);
int hegpu_ckks_bootstrap(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out, uint64_t out_stride,
                         const hegpu_bootstrap_plan* plan, const hegpu_poly_step* eval_mod, int n_steps,
                         const hegpu_linear_factor* cts, int cts_count, const hegpu_linear_factor* stc, int stc_count,
                         const uint64_t* conj_key, const uint64_t* relin_key, const uint64_t* swk_dense_to_sparse, const uint64_t* swk_sparse_to_dense,
                         int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
/* ------------------------------------------------------------------ the slim family of CKKS refreshes (slim_bootstrapping,
 * HELogicOperator<CKKS>::bit_bootstrapping and the *_bootstrapping gates, eprint 2024/767): SlotToCoeff FIRST at the bottom of
 * the chain, the raise, CoeffToSlot, the REAL parts only, ONE EvalMod-like polynomial.  One function family:
 *   alpha + A cos(2 pi (K u - phi)),  K u = I + a / ratio
 *   function   ratio        phi    A        alpha
 *   slim       config (256) 1/4    1 / 2 pi 0       sin(2 pi z / rho) / 2 pi, relabelled by 1 / rho (rho = ratio): f(z) of the
 *                                                   regular refresh
 *   bit        2            1/2    1/2      1/2     b for b in {0, 1}
 *   AND        3            2/3    2/3      1/3     with s = a + b in {0, 1, 2}: the gate's value
 *   OR         3            1/2    2/3      2/3
 *   XOR        3            1/3    2/3      1/3
 *   NAND       3            1/6    2/3      2/3
 *   NOR        3            0      2/3      1/3
 *   XNOR       3            5/6    2/3      2/3
 *
 * TRIG PLAN.  hegpu_eval_trig_plan_* is hegpu_eval_mod_plan_* with the phase, the amplitude and the offset as arguments
 * (host only): the interpolant of g(u) = c cos(2 pi (K u - phase) / 2^r), c = amplitude^(1 / 2^r), then r double-angle
 * steps; the last tail constant is (amplitude - offset) at the step's scale (any sign, or zero); with double_angle == 0 the
 * offset is added to Chebyshev coefficient 0.  (1/4, 1 / 2 pi, 0) is hegpu_eval_mod_plan_*, step for step.
 * HEGPU_E_INVALID: what hegpu_eval_mod_plan_* refuses, amplitude <= 0, a non-finite phase, amplitude or offset.
 *
 * PLAN.  hegpu_slim_bootstrap_plan_fill is host only.  The input has P_stc + 1 limbs (in_level = stc_pieces) and scale D:
 *   factor g of SlotToCoeff is encoded at stc_scale[g] (level in_level - g) and leaves the label stc_label[g]; the last is
 *   q_0 / ratio to the rounding of doubles, at level 0: no pre-multiplier;
 *   the raised ciphertext (level cts_level) is labelled raise_scale = q_0 K;
 *   factor f of CoeffToSlot is encoded at cts_scale[f] (level cts_level - f); cts_label[last] = eval_in_scale is
 *   q_(eval_level) to the rounding of doubles, eval_level = cts_level - cts_pieces - 1 (the real part drops a limb);
 *   the trig plan hegpu_eval_trig_plan_*(K, degree, double_angle, phase, amplitude, offset, eval_level, eval_in_scale,
 *   eval_target_scale) ends at out_level = eval_level - bit_length(degree) - double_angle with eval_out_scale;
 *   out_scale = eval_out_scale / ratio if config->arithmetic, else eval_out_scale.
 * HEGPU_E_INVALID, *plan untouched: fewer levels than cts_pieces + 1 + bit_length(degree) + double_angle and one limb left,
 * a chain of fewer than stc_pieces + 1 limbs, ratio < 2, piece counts outside [2, 5], a factor scale below 1, what
 * hegpu_eval_trig_plan_* refuses. */
int hegpu_eval_trig_plan_size(int K, int degree, int double_angle, double phase, double amplitude, double offset, int level,
                              double scale, double target_scale, const uint64_t* primes, int n_primes, int* n_steps);
int hegpu_eval_trig_plan_fill(int K, int degree, int double_angle, double phase, double amplitude, double offset, int level,
                              double scale, double target_scale, const uint64_t* primes, int n_primes,
                              hegpu_poly_step* steps, int n_steps);
typedef struct hegpu_slim_bootstrap_config {
    /* scale: D, the caller's scale; ratio: q_0 / (the scale of the coefficients at the raise): 256 by default for slim, 2 for
     * bits, 3 for gates */
    double scale, ratio;
    double phase, amplitude, offset;
    int32_t K, degree, double_angle;
    int32_t cts_level, cts_pieces, stc_pieces;
    int32_t arithmetic; /* 1: out_scale = eval_out_scale / ratio (slim); 0: bit and gates */
    int32_t reserved;
} hegpu_slim_bootstrap_config;
typedef struct hegpu_slim_bootstrap_plan {
    int32_t in_level, stc_pieces, cts_level, cts_pieces, eval_level, out_level;
    int32_t K, degree, double_angle;
    int32_t reserved;
    double stc_scale[5], stc_label[5]; /* factor g's diagonals (level in_level - g) and the label after it */
    double raise_scale; /* q_0 K */
    double cts_scale[5], cts_label[5];
    double ratio, phase, amplitude, offset;
    double eval_in_scale, eval_target_scale, eval_out_scale;
    double out_scale;
} hegpu_slim_bootstrap_plan;
int hegpu_slim_bootstrap_plan_fill(const hegpu_slim_bootstrap_config* config, const uint64_t* primes, int n_primes,
                                   hegpu_slim_bootstrap_plan* plan);
/* The real half of hegpu_ckks_conj_split alone: out = x + xc on the Q - out_depth kept limbs, both parts, one read of each
 * input and one write.  Bit-identical to conj_split's out0 and to hegpu_addition on the kept limbs.  out may be x itself
 * when out_depth == depth and out_stride == x_stride (in place).  Every refusal comes before the device is touched.
 * HEGPU_E_INVALID, out untouched: out overlapping xc, or x in any other way; out_depth < depth or >= Q; batch < 1. */
int hegpu_ckks_conj_real(hegpu_context* ctx, const uint64_t* x, uint64_t x_stride, const uint64_t* xc, uint64_t xc_stride,
                         uint64_t* out, uint64_t out_stride, int depth, int out_depth, int batch, hegpu_stream stream);
/* SEQUENCE.  ct (and ct2 for a gate, else NULL): [2][stc_pieces + 1][N] per item.  The launches, all on `stream`, nothing
 * allocated: with ct2 one addition of the two into the workspace -> per SlotToCoeff factor hegpu_ckks_linear_transform +
 * hegpu_ckks_rescale_inplace, down to level 0 -> hegpu_ckks_mod_raise to plan->cts_level -> per CoeffToSlot factor the same
 * pair -> hegpu_ckks_apply_galois (2N - 1, conj_key) -> hegpu_ckks_conj_real dropping one limb -> ONE hegpu_ckks_poly_eval
 * of trig at batch `batch` into out.  Bit-identical to that chain of single entries (the sum: hegpu_addition; a factor with
 * giant_parent: hegpu_ckks_linear_transform_chained, bit-identical to the same composition of single entries).  No switch
 * keys: a sparse secret is the caller's business.  out needs room for [2][out_level + 1 + rescale_after of trig's last
 * step][N] per item and holds [2][out_level + 1][N] on return, at depth Q - 1 - out_level and scale plan->out_scale.
 * HEGPU_E_INVALID before anything is queued, out untouched: a plan, trig plan or factor list that does not fit the context
 * or one another, a workspace below hegpu_ckks_slim_bootstrap_workspace_bytes (0 for arguments it cannot size; it has no row
 * in the HEGPU_OP_* table), out overlapping ct, ct2 or the workspace, ct2 overlapping the workspace, null pointers,
 * batch < 1. */
size_t hegpu_ckks_slim_bootstrap_workspace_bytes(const hegpu_context* ctx, const hegpu_slim_bootstrap_plan* plan,
                                                 const hegpu_poly_step* trig, int n_steps, const hegpu_linear_factor* cts,
                                                 int cts_count, const hegpu_linear_factor* stc, int stc_count, int batch);
int hegpu_ckks_slim_bootstrap(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, const uint64_t* ct2,
                              uint64_t ct2_stride, uint64_t* out, uint64_t out_stride,
                              const hegpu_slim_bootstrap_plan* plan, const hegpu_poly_step* trig, int n_steps,
                              const hegpu_linear_factor* cts, int cts_count, const hegpu_linear_factor* stc, int stc_count,
                              const uint64_t* conj_key, const uint64_t* relin_key, int batch, void* ws, size_t ws_bytes,
                              hegpu_stream stream);
/* multiply_bfv (src/lib/host/bfv/operator.cu:336-430): coefficient domain,
 * ct [2][Q][N] x [2][Q][N] -> out [3][Q][N] */
int hegpu_bfv_multiply(hegpu_context* ctx, const uint64_t* ct1, uint64_t ct1_stride, const uint64_t* ct2,
                       uint64_t ct2_stride, uint64_t* out, uint64_t out_stride, int batch, void* ws,
                       size_t ws_bytes, hegpu_stream stream);
/* relinearize_seal_method_inplace (bfv/operator.cu:505-583) */
int hegpu_bfv_relinearize_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t ct_stride,
                                  const uint64_t* relin_key, int batch, void* ws, size_t ws_bytes,
                                  hegpu_stream stream);
/* apply_galois_method_I (bfv/operator.cu:771-864); the result buffer must not contain the input (as above) */
int hegpu_bfv_apply_galois(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride, uint64_t* out,
                           uint64_t out_stride, const uint64_t* galois_key, int galois_elt, int batch, void* ws,
                           size_t ws_bytes, hegpu_stream stream);

/* ---- key generation, encryption, decryption (key-switching method I) ----
 * The random values are the backend's own: a ChaCha20 counter-mode PRF keyed by a 256-bit seed
 * (csrc/drbg.hpp; the reference's rngongpu::RNG<AES> is AES-CTR seeded from RAND_bytes and cannot be
 * reproduced, only its distributions: uniform mod q_i, rounded Gaussian sigma = 3.2 clipped at
 * 6 sigma, uniform ternary; src/include/heongpu/util/random.cuh:52-708).  Workspaces:
 * hegpu_workspace_bytes(ctx, HEGPU_OP_KEYGEN_* / HEGPU_OP_CKKS_ENCRYPT, 0, 1).  All keys NTT domain. */
typedef struct hegpu_rng hegpu_rng;
/* 256 bits from the operating system (getrandom): the constructor to use for real keys */
int hegpu_rng_create_from_entropy(hegpu_rng** out);
/* caller-provided 256-bit seed (e.g. from an HSM or a KDF) */
int hegpu_rng_create_seeded(const uint8_t seed[32], hegpu_rng** out);
/* REPRODUCIBLE TESTS ONLY -- a 64-bit seed is brute-forceable: key words 0,1 = seed, rest zero */
int hegpu_rng_create(uint64_t seed, hegpu_rng** out);
/* the PRF itself (host side): first 128 bits of the ChaCha20 block with counter = index, nonce =
 * stream; pinned by the RFC 8439 section 2.3.2 vector in tests/test_cabi.py */
int hegpu_drbg_block(const uint8_t key[32], uint64_t stream, uint64_t index, uint32_t out[4]);
void hegpu_rng_destroy(hegpu_rng* rng);
/* HEKeyGenerator::generate_secret_key_v2 (src/lib/host/ckks/keygenerator.cu:85-160):
 * ternary with exactly hamming_weight non-zeros; sk [Q'][N].  Synchronises the stream once. */
int hegpu_generate_secret_key(hegpu_context* ctx, hegpu_rng* rng, int hamming_weight, uint64_t* sk, void* ws,
                              size_t ws_bytes, hegpu_stream stream);
/* generate_public_key (keygenerator.cu:167-240, kernel/keygeneration.cu:93-116); pk [2][Q'][N] */
int hegpu_generate_public_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, uint64_t* pk, void* ws,
                              size_t ws_bytes, hegpu_stream stream);
/* generate_relin_key_method_I / _II (keygenerator.cu:242-414, keygeneration.cu:145-185, 584-629);
 * rk [d][2][Q'][N], d = Q (method I, P_size == 1) or the number of digits of the depth-0 partition
 * (method II: ceil(Q / P_size) for CKKS, ceil(Q / 2) for BFV) */
int hegpu_generate_relin_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, uint64_t* rk, void* ws,
                             size_t ws_bytes, hegpu_stream stream);
/* HEKeyGenerator::generate_switch_key (ckks/keygenerator.cu:996-1250, switchkey_gen_kernel /
 * switchkey_gen_II_kernel keygeneration.cu:896-989): key under new_sk that carries old_sk; layout of a
 * relinearisation key */
int hegpu_generate_switch_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* new_sk, const uint64_t* old_sk,
                              uint64_t* swk, void* ws, size_t ws_bytes, hegpu_stream stream);
/* generate_galois_key_method_I / _II, one element (keygenerator.cu:415-990, galoiskey_gen_kernel /
 * galoiskey_gen_II_kernel keygeneration.cu:742-858) */
int hegpu_generate_galois_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, int galois_elt, uint64_t* gk,
                              void* ws, size_t ws_bytes, hegpu_stream stream);
/* HEEncryptor<CKKS>::encrypt_ckks (src/lib/host/ckks/encryptor.cu:36-110); plain [Q][N], ct [2][Q][N] */
int hegpu_ckks_encrypt(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* pk, const uint64_t* plain, uint64_t* ct,
                       void* ws, size_t ws_bytes, hegpu_stream stream);
/* HEDecryptor<CKKS>::decrypt_ckks (src/lib/host/ckks/decryptor.cu:38-58); plain [Q-depth][N] */
int hegpu_ckks_decrypt(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, int depth, uint64_t* plain,
                       hegpu_stream stream);
/* HEEncryptor<BFV>::encrypt_bfv (src/lib/host/bfv/encryptor.cu:39-108, kernel/encryption.cu:91-179):
 * plain [N] residues mod t (what the batch encoder produces), ct [2][Q][N] coefficient domain */
int hegpu_bfv_encrypt(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* pk, const uint64_t* plain, uint64_t* ct,
                      void* ws, size_t ws_bytes, hegpu_stream stream);
/* HEDecryptor<BFV>::decrypt_bfv (src/lib/host/bfv/decryptor.cu:36-120, kernel/decryption.cu:10-120);
 * coefficient-domain 2-part ciphertext, plain [N] mod t.  Workspace HEGPU_OP_BFV_DECRYPT. */
int hegpu_bfv_decrypt(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, uint64_t* plain, void* ws,
                      size_t ws_bytes, hegpu_stream stream);

/* ---- N-out-of-N multiparty protocol: collective key generation and decryption ----
 * HEMultiPartyManager<CKKS|BFV> (src/lib/host/{ckks,bfv}/mpcmanager.cu, kernel/keygeneration.cu:118-462, 861-894).
 * Every party i holds a secret key s_i; the collective keys are keys under s = sum of the s_i and have exactly the
 * layout of hegpu_generate_public_key / _relin_key / _galois_key, so the evaluator takes them unchanged.  Nobody ever
 * holds s.  Shares are plain device buffers; moving them between parties is the caller's business.
 *   crs  the generator EVERY party seeds identically (public): it draws the common `a` polynomials.  Parties must
 *        make the same crs calls in the same order.
 *   rng  the party's PRIVATE generator: errors and the ephemeral secret u_i.
 * crs and rng must be different objects (HEGPU_E_INVALID otherwise: a private error drawn from the public stream
 * would hand s_i to everyone).  All polynomials NTT domain over Q' = Q u P unless said otherwise.
 * SECURITY: as in the reference, a decryption share carries only a fresh sigma = 3.2 error and NO smudging noise;
 * shares of many decryptions of related ciphertexts leak about s_i.  Key-share workspaces:
 * hegpu_workspace_bytes(ctx, HEGPU_OP_MPC_KEY_SHARE, 0, 1). */
/* generate_public_key_stage1 (ckks/mpcmanager.cu:36-90, bfv :21-75; publickey_gen_kernel with the common a):
 * share [2][Q'][N] = (-(a * s_i + e_i), a) */
int hegpu_mpc_public_key_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk, uint64_t* share,
                               void* ws, size_t ws_bytes, hegpu_stream stream);
/* generate_relin_key_method_I_stage_1 / _II_stage_1 (ckks/mpcmanager.cu:121-229, 346-462, bfv :108-216, 334-443;
 * multi_party_relinkey_piece_method_I / _II_stage_I_kernel keygeneration.cu:190-278).  Round 1, per digit d with
 * gadget term w_d: share [d][2][Q'][N] = (-(u_i * a_d) + s_i * w_d + e0, s_i * a_d + e1).  u_out [Q'][N] receives
 * the party's ephemeral ternary secret u_i: keep it private, hand it to round 2, then discard it. */
int hegpu_mpc_relin_key_share_round1(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk,
                                     uint64_t* u_out, uint64_t* share, void* ws, size_t ws_bytes, hegpu_stream stream);
/* generate_relin_key_method_I_stage_3 / _II_stage_3 (ckks/mpcmanager.cu:231-344, 464-582;
 * multi_party_relinkey_piece_method_I_II_stage_II_kernel keygeneration.cu:280-319).  Round 2 from round1_sum =
 * hegpu_mpc_accumulate(HEGPU_MPC_RELIN_ROUND1) = (h0_d, h1_d): share = (s_i * h0_d + e2, (u_i - s_i) * h1_d + e3) */
int hegpu_mpc_relin_key_share_round2(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, const uint64_t* u,
                                     const uint64_t* round1_sum, uint64_t* share, void* ws, size_t ws_bytes,
                                     hegpu_stream stream);
/* generate_galois_key_method_I / _II_stage_1, one element (ckks/mpcmanager.cu:751-1308, bfv :724-1263):
 * hegpu_generate_galois_key for s_i with the common a_d; share [d][2][Q'][N] */
int hegpu_mpc_galois_key_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk, int galois_elt,
                               uint64_t* share, void* ws, size_t ws_bytes, hegpu_stream stream);
/* generate_public_key_stage2, generate_relin_key_stage_2, generate_galois_key_stage_2 (ckks/mpcmanager.cu:92-119,
 * 584-657, 1310-1481; threshold_pk_addition, multi_party_relinkey_method_I_stage_I_kernel,
 * multi_party_galoiskey_method_I_II_kernel keygeneration.cu:118-140, 321-403, 861-894 -- one launch per share
 * there, one launch for up to 16 shares here).  shares: HOST array of k >= 1 DEVICE pointers; out must be none of them.
 *   HEGPU_MPC_PUBLIC_KEY    pk = (sum share_i[0], a)               out [2][Q'][N]
 *   HEGPU_MPC_GALOIS_KEY    gk_d = (sum share_i[d][0], a_d)        out [d][2][Q'][N]
 *   HEGPU_MPC_RELIN_ROUND1  (h0_d, h1_d) = sums of both parts      out [d][2][Q'][N] */
enum { HEGPU_MPC_PUBLIC_KEY = 0, HEGPU_MPC_GALOIS_KEY = 1, HEGPU_MPC_RELIN_ROUND1 = 2 };
int hegpu_mpc_accumulate(hegpu_context* ctx, const uint64_t* const* shares, int k, int layout, uint64_t* out,
                         hegpu_stream stream);
/* generate_relin_key_stage_4 (ckks/mpcmanager.cu:659-749; multi_party_relinkey_method_I_stage_II_kernel
 * keygeneration.cu:405-462): rk_d = (sum_i (share2_i[d][0] + share2_i[d][1]), h1_d), so that
 * rk_d[0] + s * rk_d[1] = s^2 * w_d + noise, the relation hegpu_generate_relin_key's keys satisfy */
int hegpu_mpc_relin_key_finish(hegpu_context* ctx, const uint64_t* const* round2_shares, int k,
                               const uint64_t* round1_sum, uint64_t* rk, hegpu_stream stream);
/* Collective decryption of 2-part ciphertexts, batched: item b of ct at ct + b * ct_stride.
 * partial_decrypt_stage_1 (ckks/mpcmanager.cu:1483-1539: product, error, NTT, `addition`, copy of c0 -- five
 * launches and a 2-part result): share [batch][Q - depth][N], item b = h_i = c1_b * s_i + NTT(e_b) ALONE (half the
 * reference's share; c0 stays with the ciphertext), every item with an error of its own.
 * partial_decrypt_stage_2 (:1541-1573: k `addition` launches over a temporary): plain [batch][Q - depth][N], item b =
 * c0_b + sum_i share_i[b], one launch for up to 16 shares.  shares: HOST array of k >= 1 DEVICE pointers. */
int hegpu_mpc_ckks_decrypt_share(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* ct, uint64_t ct_stride,
                                 const uint64_t* sk, int depth, uint64_t* share, int batch, hegpu_stream stream);
int hegpu_mpc_ckks_decrypt_merge(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride,
                                 const uint64_t* const* shares, int k, int depth, uint64_t* plain, int batch,
                                 hegpu_stream stream);
/* The same for BFV (bfv/mpcmanager.cu:1440-1519, 1521-1561), coefficient-domain ciphertexts: share [batch][Q][N],
 * item b = INTT(NTT(c1_b) * s_i) + e_b; plain [batch][N] mod t = the scale-and-round of hegpu_bfv_decrypt applied
 * to c0_b + sum_i share_i[b] in the same launch.  Workspace HEGPU_OP_MPC_BFV_DECRYPT_MERGE (used beyond 16 shares). */
int hegpu_mpc_bfv_decrypt_share(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* ct, uint64_t ct_stride,
                                const uint64_t* sk, uint64_t* share, int batch, hegpu_stream stream);
int hegpu_mpc_bfv_decrypt_merge(hegpu_context* ctx, const uint64_t* ct, uint64_t ct_stride,
                                const uint64_t* const* shares, int k, uint64_t* plain, int batch, void* ws,
                                size_t ws_bytes, hegpu_stream stream);

/* ---- collective refresh ("distributed bootstrapping") ----
 * HEMultiPartyManager::distributed_bootstrapping_participant / _coordinator (ckks/mpcmanager.cu:1575-1903,
 * bfv/mpcmanager.cu:1563-1752; kernels decryption.cu:480-667): the parties re-encrypt a ciphertext they can only decrypt
 * together, without anybody seeing the plaintext -- the one operation of this library that brings an exhausted
 * ciphertext (CKKS: last level; BFV: noise budget spent) back.  Batched like collective decryption: item b of ct at
 * ct + b * ct_stride, one `a`, one mask and one pair of errors per item.  crs and rng as above (the same object for
 * both: HEGPU_E_INVALID).  DRAW ORDER: every item takes one stream of crs -- item b's `a` is the b-th draw of Q limbs --
 * and three of rng (e0, e1, mask), so a batch of B items draws exactly what B calls of one item draw, in order; the
 * parties and the coordinator must start from equally advanced crs generators.  Workspaces: HEGPU_OP_MPC_REFRESH_SHARE (zero bytes: ws may be NULL) / _MERGE.
 * HEGPU_E_INVALID: crs == rng, null pointers with batch > 0, k < 1, wrong scheme, depth out of range, the mask rule
 * below, `out` overlapping the input or a share.  batch == 0: no-op, returns 0.
 * SECURITY: as for collective decryption, the errors are fresh sigma = 3.2 samples and there is NO smudging noise.
 *
 * CKKS (NTT domain; input [2][l][N] at `depth`, l = Q - depth; result [2][Q][N] at depth 0, scale unchanged):
 *   share [batch][l + Q][N] = ( h0 = c1 * s_i + NTT(e0 - M_i) over the l current limbs,
 *                               h1 = -(a * s_i) + NTT(e1 + M_i) over all Q limbs ),
 *   M_i an integer polynomial with coefficients uniform in [-2^(mask_bits-1), 2^(mask_bits-1)), 1 <= mask_bits <= 126
 *   (the reference: the encoding of N(0, 3.2) slot values, which hides nothing of a larger message).
 *   merge: t = c0 + sum h0_i -> INTT -> exact centred lift from q_0..q_{l-1} to q_0..q_{Q-1} -> NTT ->
 *   out = (lift + sum h1_i, a).  (The reference decodes t to doubles and encodes it again at the manager's scale:
 *   53 bits, two FFTs, right only when the ciphertext's scale is the manager's.)  With m~ the centred value of
 *   c0 + c1 s mod Q_level:  out[0] + out[1] * s = m~ + sum_i (e0_i + e1_i) in every limb.
 *   CORRECTNESS needs  k * 2^(mask_bits-1) + |m~| + 2 k B < Q_level / 2  (B = 20, the clip of an error sample): the
 *   entry knows neither k nor the message and refuses only what can never work, 2^mask_bits >= Q_level / 2.
 * BFV (coefficient domain, Q limbs; D(.) the scaled plaintext of hegpu_bfv_encrypt):
 *   share [batch][2][Q][N] = ( INTT(NTT(c1) * s_i) + e0 - D(M_i),  INTT(-(a * s_i)) + e1 + D(M_i) ), M_i uniform
 *   in [0, t)^N;  merge: m' = scale-and-round(c0 + sum h0_i), out = (sum h1_i + D(m'), INTT(a)).
 * shares: HOST array of k >= 1 DEVICE pointers; more than 16 go through in groups. */
int hegpu_mpc_ckks_refresh_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* ct,
                                 uint64_t ct_stride, const uint64_t* sk, int depth, int mask_bits, uint64_t* share,
                                 int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_mpc_ckks_refresh_merge(hegpu_context* ctx, hegpu_rng* crs, const uint64_t* ct, uint64_t ct_stride,
                                 const uint64_t* const* shares, int k, int depth, uint64_t* out, uint64_t out_stride,
                                 int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_mpc_bfv_refresh_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* ct,
                                uint64_t ct_stride, const uint64_t* sk, uint64_t* share, int batch, void* ws,
                                size_t ws_bytes, hegpu_stream stream);
int hegpu_mpc_bfv_refresh_merge(hegpu_context* ctx, hegpu_rng* crs, const uint64_t* ct, uint64_t ct_stride,
                                const uint64_t* const* shares, int k, uint64_t* out, uint64_t out_stride, int batch,
                                void* ws, size_t ws_bytes, hegpu_stream stream);

/* HEEncoder<BFV>::encode_bfv / decode_bfv (src/lib/host/bfv/encoder.cu:21-95, 213-249,
 * kernel/encoding.cu:11-41): batching over the slots of Z_t[X]/(X^N+1).  message: device int64
 * [message_size <= N] (negative values wrap mod t, missing slots are zero); plain [N] mod t. */
int hegpu_bfv_encode(hegpu_context* ctx, const int64_t* message, int message_size, uint64_t* plain,
                     hegpu_stream stream);
int hegpu_bfv_decode(hegpu_context* ctx, const uint64_t* plain, uint64_t* message, void* ws, size_t ws_bytes,
                     hegpu_stream stream);

/* HEEncoder<CKKS>::encode_ckks / decode_ckks for real vectors (src/lib/host/ckks/encoder.cu:21-160,
 * 449-513; kernel/encoding.cu:143-392).  The special FFT over the rotation group replaces
 * gpufft::GPU_Special_FFT (thirdparty/GPU-FFT, unvendored; HEAAN's fftSpecial/fftSpecialInv as the
 * root tables of encoder.cu:40-90 imply).  message: device doubles, at most N/2 slots (missing
 * slots are zero); plain [Q - depth][N], NTT domain.  FP64: results agree with the CPU oracle
 * bit for bit (same operation order, no FMA contraction); the reference's own rounding order
 * inside GPU-FFT is not known. */
int hegpu_ckks_encode(hegpu_context* ctx, const double* message, int message_size, double scale, uint64_t* plain,
                      void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_ckks_decode(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message, void* ws,
                      size_t ws_bytes, hegpu_stream stream);
/* The other encodings of HEEncoder<CKKS> (ckks/encoder.cu):
 *  _complex: vector<Complex64> into / out of the slots (:294-352, :515-584); message = N/2 (re, im) pairs
 *  _coeff:   encoding::COEFFICIENT -- the message is the polynomial itself, round(m_i * scale), at most N
 *            values (:222-261, encode_kernel_coeff_ckks_conversion encoding.cu:106-137); decoding returns the
 *            N coefficients (:586-635, decode_kernel_coeff_ckks_compose encoding.cu:387-464)
 *  _scalar:  one double (or an int64 cast to double) in every slot: the constant polynomial
 *            round(value * scale), written directly in the NTT domain (:412-446,
 *            encode_kernel_double_ckks_conversion encoding.cu:43-77) */
int hegpu_ckks_encode_complex(hegpu_context* ctx, const double* message, int message_size, double scale,
                              uint64_t* plain, void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_ckks_decode_complex(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message,
                              void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_ckks_encode_coeff(hegpu_context* ctx, const double* message, int message_size, double scale, uint64_t* plain,
                            hegpu_stream stream);
int hegpu_ckks_decode_coeff(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message,
                            void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_ckks_encode_scalar(hegpu_context* ctx, double value, double scale, uint64_t* plain, hegpu_stream stream);

/* HEDecryptor<BFV>::remainder_noise_budget, device part (src/lib/host/bfv/decryptor.cu:170-225):
 * out [Q][N] = t * (c0 + c1*s) mod q_j in the coefficient domain; the CRT composition and the
 * infinity norm are host work (include/heongpu/heongpu.hpp) */
int hegpu_bfv_noise_rns(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, uint64_t* out, hegpu_stream stream);

/* ---- ciphertext (x) plaintext
 * cipherplain_kernel (src/lib/kernel/multiplication.cu:298-311): out[z][j] = ct[z][j] * plain[j] for the
 * two parts, `limbs` limbs each, everything in the NTT domain (CKKS multiply_plain,
 * ckks/operator.cu multiply_plain_ckks).  CKKS add/sub of a plaintext is hegpu_addition on part 0. */
int hegpu_cipherplain_multiplication(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out,
                                     int limbs, hegpu_stream stream);
/* CKKS ciphertext with one real constant (HEArithmeticOperator::add_plain / sub_plain / multiply_plain with a
 * double, ckks/operator.cuh:312-390, :507-585, :812-925): value = constant * scale, rounded to the
 * nearest integer.  op 0: part 0 += value (addition_constant_plain_ckks_poly, addition.cu:219-258), 1: part 0
 * -= value (:260-300), 2: every part *= value (cipher_constant_plain_multiplication_kernel,
 * multiplication.cu:333-372).  ct, out: [parts][limbs][N], NTT domain; in place allowed. */
enum { HEGPU_CONST_ADD = 0, HEGPU_CONST_SUB = 1, HEGPU_CONST_MUL = 2 };
int hegpu_ckks_constant_op(hegpu_context* ctx, int op, const uint64_t* ct, double value, uint64_t* out, int limbs,
                           int parts, hegpu_stream stream);
/* add_constant_plain_ckks_v2 / multiply_const_plain_ckks_v2 (ckks/operator.cu:567-724, kernels
 * multiplication.cu:497-570): the Gaussian integer round(re) + round(im) i in every slot of an NTT-domain
 * ciphertext; op 0: added to part 0, op 1: every part multiplied by it.  re / im are the already scaled
 * values (the caller applies input.scale resp. the modulus factor exactly as the reference's host code does). */
int hegpu_ckks_gaussian_integer_op(hegpu_context* ctx, int op, const uint64_t* ct, double re, double im, uint64_t* out,
                                   int limbs, int parts, hegpu_stream stream);
/* HEArithmeticOperator::mult_i / div_i (cipher_mult_by_i_kernel / cipher_div_by_i_kernel,
 * multiplication.cu:441-495): every slot times +-i, no level consumed */
int hegpu_ckks_mult_i(hegpu_context* ctx, const uint64_t* ct, uint64_t* out, int limbs, int parts, int divide,
                      hegpu_stream stream);
/* addition_plain_bfv_poly / substraction_plain_bfv_poly (src/lib/kernel/addition.cu:50-176): part 0 gets
 * +-(floor(Q/t)*m + fix), part 1 is copied; plain [N] mod t, coefficient-domain ciphertext */
int hegpu_bfv_plain_addsub(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out, int sub,
                           hegpu_stream stream);
/* HEOperator<BFV>::multiply_plain_bfv (src/lib/host/bfv/operator.cu:432-503): threshold lift, NTT,
 * cipherplain product, INTT.  Workspace HEGPU_OP_BFV_MULTIPLY_PLAIN. */
/* HEArithmeticOperator<BFV>::transform_to_ntt(Plaintext) (bfv/operator.cu:1398-1431): plain [N] mod t -> [Q][N],
 * threshold lift (multiplication.cu:274-296) + forward NTT; such a plaintext multiplies an NTT-domain
 * ciphertext with hegpu_cipherplain_multiplication.  (Ciphertexts change domain with hegpu_ntt.) */
int hegpu_bfv_plain_to_ntt(hegpu_context* ctx, const uint64_t* plain, uint64_t* out, hegpu_stream stream);
/* HEArithmeticOperator<BFV>::multiply_power_of_X (negacyclic_shift_poly_coeffmod_kernel, switchkey.cu:1433-1457):
 * out = in * X^shift in the coefficient domain, [parts][limbs][N]; out must not alias in */
int hegpu_negacyclic_shift(hegpu_context* ctx, const uint64_t* in, uint64_t* out, int shift, int limbs, int parts,
                           hegpu_stream stream);
int hegpu_bfv_multiply_plain(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out, void* ws,
                             size_t ws_bytes, hegpu_stream stream);

/* ------------------------------------------------------------------ logic gates on encrypted bits (BFV / CKKS)
 * HELogicOperator<Scheme::BFV> (src/include/heongpu/host/bfv/operator.cuh:1324-2230, src/lib/host/bfv/operator.cu:1520-1575)
 * and HELogicOperator<Scheme::CKKS> (host/ckks/operator.cuh:2333-3500, src/lib/host/ckks/operator.cu:7329-7346, :8195-8225):
 * a bit is the value 0 or 1 in a slot, and every gate is  c0 * 1 + c1 * (a + b) + c2 * (a * b):
 *   AND (0,0,1)  OR (0,1,-1)  XOR (0,1,-2)  NAND (1,0,-1)  NOR (1,-1,1)  XNOR (1,-1,2)  NOT (1,-1; no b, no product)
 * The numbering is this enum's own (the TFHE gates below keep theirs: HEGPU_GATE_*). */
enum {
    HEGPU_LOGIC_AND = 0, HEGPU_LOGIC_OR = 1, HEGPU_LOGIC_XOR = 2, HEGPU_LOGIC_NAND = 3, HEGPU_LOGIC_NOR = 4,
    HEGPU_LOGIC_XNOR = 5, HEGPU_LOGIC_NOT = 6
};
enum { HEGPU_GATE_B_NONE = 0, HEGPU_GATE_B_CIPHER = 1, HEGPU_GATE_B_PLAIN = 2 }; /* the second operand of a gate */
/* The part of a gate after the product p = a * b, in ONE pass: reads a, b and p in place, writes out.  The reference
 * chains add(p, p), add(a, b), mod_drop copies, sub, negate (one_minus_cipher, ckks/operator.cu:7329-7346) and the
 * plaintext add of its encoded_constant_one_ as separate launches (host/ckks/operator.cuh:2528-3230, each "TODO: make it
 * efficient").  out = c0 * one * [part 0] + c1 * (a + b) + c2 * p over the first `limbs` limbs of both parts, canonical.
 *   a, p: [2][a_limbs / p_limbs][N] per item, each >= limbs, only the first `limbs` limbs of a part are read (CKKS: a and
 *   b sit one level above p).  b: HEGPU_GATE_B_CIPHER [2][b_limbs][N]; HEGPU_GATE_B_PLAIN, added to part 0 only: CKKS
 *   [b_limbs][N] NTT-domain residues, BFV [N] residues mod t that enter as floor(Q/t) m + fix, the residues of
 *   hegpu_bfv_plain_addsub; a plaintext shared by all items has b_stride 0.  NOT: b_kind HEGPU_GATE_B_NONE, b and p NULL.
 *   one: CKKS round(scale_one) in every NTT position (the residue hegpu_ckks_constant_op adds); BFV the scaled plaintext
 *   of m = 1 on coefficient 0 (the polynomial 1).  BFV: coefficient domain, every limb count is Q.
 * Bit-identical to the chain hegpu_addition / hegpu_ckks_constant_op / hegpu_bfv_plain_addsub on the kept limbs.
 * out may be a, or a ciphertext b, itself (same address and stride) when that operand has exactly `limbs` limbs -- BFV
 * always, a CKKS NOT.  HEGPU_E_INVALID before anything is queued (no device needed): any other overlap of out with an
 * input, an unknown gate, operands that do not fit the gate, a limb count outside [limbs, Q], 2 * batch > 65535,
 * batch < 0, scale_one not in (0, 3.4e38), the wrong scheme.  batch == 0: no-op. */
int hegpu_ckks_gate_combine(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, int a_limbs,
                            const uint64_t* b, int b_kind, uint64_t b_stride, int b_limbs, const uint64_t* p,
                            uint64_t p_stride, int p_limbs, double scale_one, uint64_t* out, uint64_t out_stride, int limbs,
                            int batch, hegpu_stream stream);
int hegpu_bfv_gate_combine(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b,
                           int b_kind, uint64_t b_stride, const uint64_t* p, uint64_t p_stride, uint64_t* out,
                           uint64_t out_stride, int batch, hegpu_stream stream);
/* The whole gate, batched (HELogicOperator::AND .. XNOR, NOT and their _inplace forms): the product sequence into the
 * workspace, then the one combine pass (AND: the pass is its copy out of the workspace); NOT is the pass alone (ws unused).
 *   b ciphertext: hegpu_ckks_multiply, _relinearize_inplace, _rescale_inplace  /  hegpu_bfv_multiply, _relinearize_inplace
 *   b plaintext:  hegpu_cipherplain_multiplication per item, _rescale_inplace  /  hegpu_bfv_multiply_plain per item
 * CKKS: a and b at `depth`, l = Q - depth limbs (a plaintext b: [l][N]); out [2][l - 1][N] per item at depth + 1 for a
 * binary gate, [2][l][N] for NOT.  EVERY gate reads the sum a + b at the product's level: the reference's ciphertext OR,
 * XOR, NOR and XNOR hand a depth-d sum and a depth-d+1 product to sub(), which throws.  BFV: everything [2][Q][N].
 * Bit-identical to the chain of the single entries.  Workspace HEGPU_OP_CKKS_LOGIC_GATE / HEGPU_OP_BFV_LOGIC_GATE.
 * HEGPU_E_INVALID before anything is queued: what the combine refuses, a short workspace, a missing key, out overlapping
 * the workspace, a CKKS binary gate on the last level. */
int hegpu_ckks_logic_gate(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b, int b_kind,
                          uint64_t b_stride, const uint64_t* relin_key, double scale_one, uint64_t* out, uint64_t out_stride,
                          int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream);
int hegpu_bfv_logic_gate(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b, int b_kind,
                         uint64_t b_stride, const uint64_t* relin_key, uint64_t* out, uint64_t out_stride, int batch, void* ws,
                         size_t ws_bytes, hegpu_stream stream);

/* ------------------------------------------------------------------ TFHE
 * Gate bootstrapping on the reference's fixed STD128 set
 * (src/lib/host/tfhe/context.cu:15-57: n=512, N=1024, k=1, l=2, Bg=2^10,
 * ks_base_bit=2, ks_length=8, NTT prime 1152921504606877697).
 * LWE ciphertexts: a [shape][n] + b [shape], int32 torus
 * (src/lib/host/tfhe/operator.cu:296-314).  Boot key: uint64 NTT domain,
 * reference layout [n][k+1][l][k+1][N] (bootstrapping.cu:1037-1041);
 * key-switch key a [N*k][ks_length][base-1][n], b [N*k][ks_length][base-1]
 * (bootstrapping.cu:1385-1412). */
typedef struct hegpu_tfhe_context hegpu_tfhe_context;
enum {
    HEGPU_GATE_NAND = 0, HEGPU_GATE_AND = 1, HEGPU_GATE_AND_FIRST_NOT = 2, HEGPU_GATE_NOR = 3,
    HEGPU_GATE_OR = 4, HEGPU_GATE_XNOR = 5, HEGPU_GATE_XOR = 6, HEGPU_GATE_NOT = 7
};
/* HEContextImpl<TFHE>::HEContextImpl (tfhe/context.cu:15-57); host only */
int hegpu_tfhe_context_create(hegpu_tfhe_context** out);
void hegpu_tfhe_context_destroy(hegpu_tfhe_context* ctx);
/* "fp" 0/1: re-encode a torus32 boot key for the FP64 blind rotate (1, read by hegpu_tfhe_prepare_bootkey);
 * "ks_batched" -1/0/1/8/12/16: key switching with that many gates per workgroup sharing the key rows: by launch
 * size (-1, default: 16 per workgroup from 48 gates per call), never, always (16), always with that many;
 * "ks_pieces" -1 / 1..64: workgroups the input-coefficient loop of a gate (or group of gates) is cut into (partial sums
 * added with integer atomics: the same bits), -1 = by launch size.
 * Defaults seeded once, at creation, from HEGPU_TFHE_FP / HEGPU_TFHE_KS_BATCHED / HEGPU_TFHE_KS_PIECES when these hold
 * whole decimal integers the setter accepts (anything else is ignored). */
int hegpu_tfhe_context_set_option(hegpu_tfhe_context* ctx, const char* name, int value);
/* "n","N","k","bk_l","bk_bg_bit","ks_base_bit","ks_length","offset","bootkey_elems",
 * "prepared_bootkey_elems","kskey_a_elems","kskey_b_elems" */
long hegpu_tfhe_context_int(const hegpu_tfhe_context* ctx, const char* name);
uint64_t hegpu_tfhe_prime(const hegpu_tfhe_context* ctx);
/* One-time conversion of a boot key (reference layout, NTT domain) into the layout the
 * blind rotate reads; `prepared` holds "prepared_bootkey_elems" uint64.  Synchronises the
 * stream once: a real key (torus32 coefficients) is re-encoded for the FP64 blind rotate,
 * any other key keeps the reference's 60-bit prime (results are identical either way). */
int hegpu_tfhe_prepare_bootkey(hegpu_tfhe_context* ctx, const uint64_t* boot_key, uint64_t* prepared,
                               hegpu_stream stream);
/* Layout of a prepared boot key: 1 = FP64, 0 = integer (its header word), -1 on ANY error.  A query only: the blind
 * rotate reads the header word on the device, in the order of the call's stream, so a buffer may be filled, copied
 * (hegpu_broadcast_bytes) or overwritten on that stream right before a gate call without any host synchronisation.
 * This call drains the device, then reads the word.  `refresh` is ignored (nothing is remembered since round 5).
 * A bootstrapping call that is handed a buffer whose header is neither layout writes no outputs and raises the context's
 * bad-key flag on the device: see hegpu_tfhe_status. */
int hegpu_tfhe_prepared_format(hegpu_tfhe_context* ctx, const uint64_t* prepared, int refresh);
/* tfhe_{nand,and,and_first_not,nor,or,xnor,xor}_pre_comp_kernel / tfhe_not_comp_kernel
 * (src/lib/kernel/bootstrapping.cu:378-660); in2_* ignored for NOT */
int hegpu_tfhe_gate_precompute(hegpu_tfhe_context* ctx, int gate, int32_t* out_a, int32_t* out_b,
                               const int32_t* in1_a, const int32_t* in1_b, const int32_t* in2_a,
                               const int32_t* in2_b, int shape, hegpu_stream stream);
/* HELogicOperator<TFHE>::bootstrapping (tfhe/operator.cu:200-270): blind rotate with
 * test vector mu = encode_to_torus32(1,8) + sample extraction; out_a [shape][k*N] */
int hegpu_tfhe_bootstrapping(hegpu_tfhe_context* ctx, const int32_t* in_a, const int32_t* in_b,
                             const uint64_t* prepared_boot_key, int32_t* out_a, int32_t* out_b, int shape,
                             hegpu_stream stream);
/* The error check after a launch that the reference does with HEONGPU_CUDA_CHECK(cudaGetLastError())
 * (src/include/heongpu/util/util.cuh:47-55), for the one error this backend can only find ON THE DEVICE: the layout of a
 * prepared boot key is read by the blind-rotate kernel itself, in stream order; a buffer that is no prepared key (header word
 * neither 0 nor 1) makes it write NO outputs and raise the context's bad-key flag.  hegpu_tfhe_status drains `stream`, then
 * returns HEGPU_E_INVALID if the flag is up -- and clears it -- else 0: bootstrapping / gate / mux call + status = the
 * error at the call that caused it.  The flag belongs to the context, not to a stream: with several streams on one
 * context, drain them all before asking.  A caller that never asks hears about it at the entry of its NEXT
 * hegpu_tfhe_bootstrapping / _gate / _mux (before anything of that call is queued); no other entry looks at the flag. */
int hegpu_tfhe_status(hegpu_tfhe_context* ctx, hegpu_stream stream);
/* HELogicOperator<TFHE>::key_switching (tfhe/operator.cu:272-294).  The output sample must not overlap the input
 * sample (HEGPU_E_INVALID): the forms that cut a gate's coefficient loop over several workgroups clear the outputs first. */
int hegpu_tfhe_key_switching(hegpu_tfhe_context* ctx, const int32_t* in_a, const int32_t* in_b, int32_t* out_a,
                             int32_t* out_b, const int32_t* ks_key_a, const int32_t* ks_key_b, int shape,
                             hegpu_stream stream);
/* HELogicOperator<TFHE>::{NAND,AND,NOR,OR,XNOR,XOR} (tfhe/operator.cuh:53-640):
 * precompute -> bootstrapping -> key switching.  ws: (n + k*N + 2) * shape int32. */
int hegpu_tfhe_gate(hegpu_tfhe_context* ctx, int gate, const int32_t* in1_a, const int32_t* in1_b,
                    const int32_t* in2_a, const int32_t* in2_b, int32_t* out_a, int32_t* out_b,
                    const uint64_t* prepared_boot_key, const int32_t* ks_key_a, const int32_t* ks_key_b, int shape,
                    void* ws, size_t ws_bytes, hegpu_stream stream);

/* ---- TFHE front end: keys, bit encryption, decryption, MUX
 * (src/lib/host/tfhe/keygenerator.cu, encryptor.cu, decryptor.cu, include/.../tfhe/operator.cuh:676-800).
 * Own DRBG as for the RLWE schemes; torus noise = scaled Irwin-Hall(16) (csrc/drbg.hpp) with the
 * reference's standard deviations (tfhe/context.cu:39-42).  Keys are binary. */
int hegpu_tfhe_generate_secret_key(hegpu_tfhe_context* ctx, hegpu_rng* rng, int32_t* lwe_key /* [n] */,
                                   int32_t* tlwe_key /* [k*N] */, hegpu_stream stream);
/* boot_key: reference layout [n][k+1][l][k+1][N] (NTT domain), then hegpu_tfhe_prepare_bootkey;
 * ks_a [N*k][ks_length][base-1][n], ks_b [N*k][ks_length][base-1]; ws: N uint64 */
int hegpu_tfhe_generate_bootstrapping_key(hegpu_tfhe_context* ctx, hegpu_rng* rng, const int32_t* lwe_key,
                                          const int32_t* tlwe_key, uint64_t* boot_key, int32_t* ks_a, int32_t* ks_b,
                                          void* ws, size_t ws_bytes, hegpu_stream stream);
/* LWE encryption of torus32 messages (a bit is +-1/8 = +-2^29): a [shape][n], b [shape] */
int hegpu_tfhe_encrypt(hegpu_tfhe_context* ctx, hegpu_rng* rng, const int32_t* lwe_key, const int32_t* messages,
                       int shape, int32_t* out_a, int32_t* out_b, hegpu_stream stream);
/* phase = b - <a, key>; the bit is phase > 0 */
int hegpu_tfhe_decrypt_phase(hegpu_tfhe_context* ctx, const int32_t* lwe_key, const int32_t* a, const int32_t* b,
                             int shape, int32_t* phase, hegpu_stream stream);
/* MUX(in1, in2, control) = OR(AND(control, in1), AND(NOT control, in2)) with two bootstraps and one
 * key switch (operator.cuh:688-800).  ws: (n + 1 + 2*(k*N + 1)) * shape int32. */
int hegpu_tfhe_mux(hegpu_tfhe_context* ctx, const int32_t* in1_a, const int32_t* in1_b, const int32_t* in2_a,
                   const int32_t* in2_b, const int32_t* c_a, const int32_t* c_b, int32_t* out_a, int32_t* out_b,
                   const uint64_t* prepared_boot_key, const int32_t* ks_a, const int32_t* ks_b, int shape, void* ws,
                   size_t ws_bytes, hegpu_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HEGPU_H */
