/*
 * ref_kernels_driver.cpp -- C entry points that launch the REFERENCE's own RNS kernels (src/lib/kernel/switchkey.cu,
 * multiplication.cu, addition.cu, compiled unchanged by oracle/ref_build.py against oracle/ref_shim/) next to this
 * project's kernels, for tests/test_gpu_reference_kernels.py.  TEST INFRASTRUCTURE ONLY; own code: nothing here is
 * taken from the reference but the kernel names and parameter lists it declares in its headers.
 *
 * Every refk_* launch entry
 *   - launches ONE reference kernel on the caller's stream with the grid and block of the reference's HOST call site
 *     (src/lib/host/{ckks,bfv}/operator.cu, cited per entry), never with this project's launch shapes;
 *   - takes, next to every buffer, its length (64-bit words for data and tables, entries for Modulus64 and int
 *     arrays) and returns REFK_E_RANGE WITHOUT LAUNCHING when the index range implied by the grid and the kernel's
 *     own index arithmetic would leave any of them; REFK_E_ARG for a count <= 0 or an n_power outside 12..16;
 *   - allocates nothing and never synchronises.
 * The bounds are derived from the kernel text (file:line of the kernel is cited next to each rule).
 */
#include <cstdint>
#include <hip/hip_runtime.h>

#include <heongpu/kernel/addition.cuh>
#include <heongpu/kernel/multiplication.cuh>
#include <heongpu/kernel/switchkey.cuh>

using namespace heongpu;

enum { REFK_OK = 0, REFK_E_ARG = -1, REFK_E_RANGE = -2, REFK_E_NULL = -3, REFK_E_LAUNCH = -4 };

typedef long long i64;

#define REFK_GEOMETRY(n_power)                          \
    if ((n_power) < 12 || (n_power) > 16) return REFK_E_ARG; \
    const i64 n = ((i64) 1) << (n_power);               \
    const unsigned gx = (unsigned) (n >> 8);            \
    (void) gx
#define REFK_COUNT(v) \
    if ((v) <= 0) return REFK_E_ARG
#define REFK_NEED(ptr, len, words)                       \
    do {                                                 \
        if (!(ptr)) return REFK_E_NULL;                  \
        if ((i64) (words) > 0x7fffffffLL) return REFK_E_RANGE; /* the kernels index with int */ \
        if ((i64) (len) < (i64) (words)) return REFK_E_RANGE;  \
    } while (0)
/* after the last check of an entry: with the dry run on, a call that passed every check returns here, so the checks
 * themselves (exact lengths accepted, one word less refused) can be tested on a machine without a GPU */
#define REFK_CHECKED() \
    if (g_dry_run) return REFK_OK
#define REFK_DONE() return hipGetLastError() == hipSuccess ? REFK_OK : REFK_E_LAUNCH

static int g_dry_run = 0;

static inline hipStream_t st(void* s) { return (hipStream_t) s; }
static inline Data64* D(const uint64_t* p) { return (Data64*) p; }
static inline Modulus64* M(const void* p) { return (Modulus64*) p; }

/* words of the mod-down tables half_mod / last_q_modinv that the multi-prime kernels walk: location_ advances by
 * first_Q_prime_size - 1 - i per special prime (switchkey.cu:533, 1277, 1677, 1772) */
static inline i64 moddown_table_words(int first_Qp, int P)
{
    i64 w = 0;
    for (int i = 0; i < P; i++) w += first_Qp - 1 - i;
    return w;
}

extern "C" {

int refk_abi_version(void) { return 1; }
void refk_set_dry_run(int on) { g_dry_run = on; }

/* ------------------------------------------------------------------ host probes of the stand-in header */
void refk_host_mod(uint64_t q, uint64_t* out3)
{
    Modulus64 m(q);
    out3[0] = m.value;
    out3[1] = m.bit;
    out3[2] = m.mu;
}
uint64_t refk_host_add(uint64_t a, uint64_t b, uint64_t q) { return OPERATOR_GPU_64::add(a, b, Modulus64(q)); }
uint64_t refk_host_sub(uint64_t a, uint64_t b, uint64_t q) { return OPERATOR_GPU_64::sub(a, b, Modulus64(q)); }
uint64_t refk_host_mult(uint64_t a, uint64_t b, uint64_t q) { return OPERATOR_GPU_64::mult(a, b, Modulus64(q)); }
uint64_t refk_host_reduce_forced(uint64_t a, uint64_t q) { return OPERATOR_GPU_64::reduce_forced(a, Modulus64(q)); }
uint64_t refk_host_reduce128(uint64_t lo, uint64_t hi, uint64_t q)
{
    const Data64 v[2] = {lo, hi};
    return OPERATOR_GPU_64::reduce(v, Modulus64(q));
}

/* Modulus64 array on the device from a list of primes.  `staging` is HOST memory of 3 * count words owned by the
 * caller, filled here and copied on `stream`; it must stay alive until the stream has been synchronised. */
int refk_moduli_fill(const uint64_t* primes, int count, uint64_t* staging, i64 staging_words, void* dev_out,
                     i64 dev_entries, void* stream)
{
    REFK_COUNT(count);
    if (!primes || !staging || !dev_out) return REFK_E_NULL;
    if (staging_words < 3 * (i64) count || dev_entries < count) return REFK_E_RANGE;
    static_assert(sizeof(Modulus64) == 3 * sizeof(uint64_t), "Modulus64 is {value, bit, mu}");
    for (int i = 0; i < count; i++) {
        if (primes[i] < 2 || (primes[i] >> 62) != 0) return REFK_E_ARG;
        refk_host_mod(primes[i], staging + 3 * i);
    }
    return hipMemcpyAsync(dev_out, staging, sizeof(Modulus64) * count, hipMemcpyHostToDevice, st(stream)) == hipSuccess
               ? REFK_OK
               : REFK_E_LAUNCH;
}

/* ------------------------------------------------------------------ addition.cu */
/* addition / substraction / negation (addition.cu:10-48): location < parts * limbs * n, modulus[idy < limbs].
 * Grid dim3(n >> 8, current_decomp_count, cipher_size), 256: ckks/operator.cu:123, 214, 275; bfv/operator.cu:68, 140, 193. */
int refk_addition(int op, const uint64_t* in1, i64 in1_len, const uint64_t* in2, i64 in2_len, uint64_t* out, i64 out_len,
                  const void* modulus, i64 modulus_len, int n_power, int limbs, int parts, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(limbs);
    REFK_COUNT(parts);
    if (op < 0 || op > 2) return REFK_E_ARG;
    const i64 words = (i64) parts * limbs * n;
    REFK_NEED(in1, in1_len, words);
    if (op != 2) REFK_NEED(in2, in2_len, words);
    REFK_NEED(out, out_len, words);
    REFK_NEED(modulus, modulus_len, limbs);
    REFK_CHECKED();
    const dim3 grid(gx, limbs, parts);
    if (op == 0)
        addition<<<grid, 256, 0, st(stream)>>>(D(in1), D(in2), out, M(modulus), n_power);
    else if (op == 1)
        substraction<<<grid, 256, 0, st(stream)>>>(D(in1), D(in2), out, M(modulus), n_power);
    else
        negation<<<grid, 256, 0, st(stream)>>>(D(in1), out, M(modulus), n_power);
    REFK_DONE();
}

/* addition_plain_bfv_poly / substraction_plain_bfv_poly (addition.cu:50-85, 113-147): plain[idx < n],
 * coeffdiv_plain[block_y < Q], location < cipher_size * Q * n.
 * Grid dim3(n >> 8, Q_size, cipher_size), 256: bfv/operator.cu:236, 296. */
int refk_bfv_plain_addsub(int sub, const uint64_t* cipher, i64 cipher_len, const uint64_t* plain, i64 plain_len,
                          uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len, uint64_t plain_mod,
                          uint64_t Q_mod_t, uint64_t upper_threshold, const uint64_t* coeffdiv_plain, i64 coeffdiv_len,
                          int n_power, int Q_size, int cipher_size, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(Q_size);
    REFK_COUNT(cipher_size);
    if (plain_mod < 2) return REFK_E_ARG;
    const i64 words = (i64) cipher_size * Q_size * n;
    REFK_NEED(cipher, cipher_len, words);
    REFK_NEED(plain, plain_len, n);
    REFK_NEED(out, out_len, words);
    REFK_NEED(modulus, modulus_len, Q_size);
    REFK_NEED(coeffdiv_plain, coeffdiv_len, Q_size);
    REFK_CHECKED();
    const dim3 grid(gx, Q_size, cipher_size);
    const Modulus64 t(plain_mod);
    if (sub)
        substraction_plain_bfv_poly<<<grid, 256, 0, st(stream)>>>(D(cipher), D(plain), out, M(modulus), t, Q_mod_t,
                                                                  upper_threshold, D(coeffdiv_plain), n_power);
    else
        addition_plain_bfv_poly<<<grid, 256, 0, st(stream)>>>(D(cipher), D(plain), out, M(modulus), t, Q_mod_t,
                                                              upper_threshold, D(coeffdiv_plain), n_power);
    REFK_DONE();
}

/* addition_constant_plain_ckks_poly / substraction_constant_plain_ckks_poly (addition.cu:219-307) and
 * cipher_constant_plain_multiplication_kernel (multiplication.cu:333-372): location < parts * limbs * n.
 * Grid dim3(n >> 8, current_decomp_count, cipher_size), 256 with two_pow_64 = 2^64: ckks/operator.cu:400, 533; the
 * product is launched with 2 in z (ckks/operator.cu:884), `parts` here. */
int refk_ckks_constant_op(int op, const uint64_t* in, i64 in_len, double value, uint64_t* out, i64 out_len,
                          const void* modulus, i64 modulus_len, int n_power, int limbs, int parts, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(limbs);
    REFK_COUNT(parts);
    if (op < 0 || op > 2) return REFK_E_ARG;
    const i64 words = (i64) parts * limbs * n;
    REFK_NEED(in, in_len, words);
    REFK_NEED(out, out_len, words);
    REFK_NEED(modulus, modulus_len, limbs);
    REFK_CHECKED();
    const dim3 grid(gx, limbs, parts);
    const double two_pow_64 = 18446744073709551616.0;
    if (op == 0)
        addition_constant_plain_ckks_poly<<<grid, 256, 0, st(stream)>>>(D(in), value, out, M(modulus), two_pow_64, n_power);
    else if (op == 1)
        substraction_constant_plain_ckks_poly<<<grid, 256, 0, st(stream)>>>(D(in), value, out, M(modulus), two_pow_64,
                                                                            n_power);
    else
        cipher_constant_plain_multiplication_kernel<<<grid, 256, 0, st(stream)>>>(D(in), value, out, M(modulus), two_pow_64,
                                                                                  n_power);
    REFK_DONE();
}

/* ------------------------------------------------------------------ multiplication.cu */
/* cross_multiplication (multiplication.cu:102-126): in1 / in2 up to location + decomp_size * n, out up to
 * location + 2 * decomp_size * n, location < decomp_size * n.
 * Grid dim3(n >> 8, decomp_size, 1), 256: ckks/operator.cu:822, bfv/operator.cu:399. */
int refk_cross_multiplication(const uint64_t* in1, i64 in1_len, const uint64_t* in2, i64 in2_len, uint64_t* out,
                              i64 out_len, const void* modulus, i64 modulus_len, int n_power, int decomp_size,
                              void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(decomp_size);
    REFK_NEED(in1, in1_len, 2 * (i64) decomp_size * n);
    REFK_NEED(in2, in2_len, 2 * (i64) decomp_size * n);
    REFK_NEED(out, out_len, 3 * (i64) decomp_size * n);
    REFK_NEED(modulus, modulus_len, decomp_size);
    REFK_CHECKED();
    cross_multiplication<<<dim3(gx, decomp_size, 1), 256, 0, st(stream)>>>(D(in1), D(in2), out, M(modulus), n_power,
                                                                          decomp_size);
    REFK_DONE();
}

/* fast_convertion (multiplication.cu:10-100): in1 / in2 [2][ibase][n], out1 [4][ibase + obase][n]; the register
 * arrays hold MAX_BSK_SIZE words and temp2[obase_size] is written (:56), so ibase <= 64 and obase <= 63.
 * Grid dim3(n >> 8, 4, 1), 256: bfv/operator.cu:364. */
int refk_fast_convertion(const uint64_t* in1, i64 in1_len, const uint64_t* in2, i64 in2_len, uint64_t* out, i64 out_len,
                         const void* ibase, i64 ibase_len, const void* obase, i64 obase_len, uint64_t m_tilde,
                         uint64_t inv_prod_q_mod_m_tilde, const uint64_t* inv_m_tilde_mod_Bsk, i64 len_a,
                         const uint64_t* prod_q_mod_Bsk, i64 len_b, const uint64_t* base_change_matrix_Bsk, i64 len_c,
                         const uint64_t* base_change_matrix_m_tilde, i64 len_d,
                         const uint64_t* inv_punctured_prod_mod_base_array, i64 len_e, int n_power, int ibase_size,
                         int obase_size, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(ibase_size);
    REFK_COUNT(obase_size);
    if (ibase_size > MAX_BSK_SIZE || obase_size > MAX_BSK_SIZE - 1 || m_tilde < 2) return REFK_E_ARG;
    REFK_NEED(in1, in1_len, 2 * (i64) ibase_size * n);
    REFK_NEED(in2, in2_len, 2 * (i64) ibase_size * n);
    REFK_NEED(out, out_len, 4 * (i64) (ibase_size + obase_size) * n);
    REFK_NEED(ibase, ibase_len, ibase_size);
    REFK_NEED(obase, obase_len, obase_size);
    REFK_NEED(inv_m_tilde_mod_Bsk, len_a, obase_size);
    REFK_NEED(prod_q_mod_Bsk, len_b, obase_size);
    REFK_NEED(base_change_matrix_Bsk, len_c, (i64) ibase_size * obase_size);
    REFK_NEED(base_change_matrix_m_tilde, len_d, ibase_size);
    REFK_NEED(inv_punctured_prod_mod_base_array, len_e, ibase_size);
    REFK_CHECKED();
    fast_convertion<<<dim3(gx, 4, 1), 256, 0, st(stream)>>>(
        D(in1), D(in2), out, M(ibase), M(obase), Modulus64(m_tilde), inv_prod_q_mod_m_tilde, D(inv_m_tilde_mod_Bsk),
        D(prod_q_mod_Bsk), D(base_change_matrix_Bsk), D(base_change_matrix_m_tilde), D(inv_punctured_prod_mod_base_array),
        n_power, ibase_size, obase_size);
    REFK_DONE();
}

/* fast_floor (multiplication.cu:128-272): in [3][ibase + obase][n], out [3][ibase][n]; temp4[ibase_size] is written
 * (:219), so ibase <= 63, obase <= 64 and obase >= 2 (obase - 1 primes of B).
 * Grid dim3(n >> 8, 3, 1), 256: bfv/operator.cu:416. */
int refk_fast_floor(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, const void* ibase, i64 ibase_len,
                    const void* obase, i64 obase_len, uint64_t plain_modulus,
                    const uint64_t* inv_punctured_prod_mod_base_array, i64 len_a, const uint64_t* base_change_matrix_Bsk,
                    i64 len_b, const uint64_t* inv_prod_q_mod_Bsk, i64 len_c,
                    const uint64_t* inv_punctured_prod_mod_B_array, i64 len_d, const uint64_t* base_change_matrix_q,
                    i64 len_e, const uint64_t* base_change_matrix_msk, i64 len_f, uint64_t inv_prod_B_mod_m_sk,
                    const uint64_t* prod_B_mod_q, i64 len_g, int n_power, int ibase_size, int obase_size, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(ibase_size);
    REFK_COUNT(obase_size);
    if (ibase_size > MAX_BSK_SIZE - 1 || obase_size > MAX_BSK_SIZE || obase_size < 2 || plain_modulus < 2) return REFK_E_ARG;
    REFK_NEED(in, in_len, 3 * (i64) (ibase_size + obase_size) * n);
    REFK_NEED(out, out_len, 3 * (i64) ibase_size * n);
    REFK_NEED(ibase, ibase_len, ibase_size);
    REFK_NEED(obase, obase_len, obase_size);
    REFK_NEED(inv_punctured_prod_mod_base_array, len_a, ibase_size);
    REFK_NEED(base_change_matrix_Bsk, len_b, (i64) ibase_size * obase_size);
    REFK_NEED(inv_prod_q_mod_Bsk, len_c, obase_size);
    REFK_NEED(inv_punctured_prod_mod_B_array, len_d, obase_size - 1);
    REFK_NEED(base_change_matrix_q, len_e, (i64) ibase_size * (obase_size - 1));
    REFK_NEED(base_change_matrix_msk, len_f, obase_size - 1);
    REFK_NEED(prod_B_mod_q, len_g, ibase_size);
    REFK_CHECKED();
    fast_floor<<<dim3(gx, 3, 1), 256, 0, st(stream)>>>(
        D(in), out, M(ibase), M(obase), Modulus64(plain_modulus), D(inv_punctured_prod_mod_base_array),
        D(base_change_matrix_Bsk), D(inv_prod_q_mod_Bsk), D(inv_punctured_prod_mod_B_array), D(base_change_matrix_q),
        D(base_change_matrix_msk), inv_prod_B_mod_m_sk, D(prod_B_mod_q), n_power, ibase_size, obase_size);
    REFK_DONE();
}

/* threshold_kernel (multiplication.cu:274-296): plain_in[idx < n], output < decomp_size * n,
 * plain_upper_half_increment[block_y].  Grid dim3(n >> 8, Q_size, 1), 256: bfv/operator.cu:454, 1409. */
int refk_threshold(const uint64_t* plain, i64 plain_len, uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len,
                   const uint64_t* upper_half_increment, i64 inc_len, uint64_t upper_half_threshold, int n_power,
                   int decomp_size, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(decomp_size);
    REFK_NEED(plain, plain_len, n);
    REFK_NEED(out, out_len, (i64) decomp_size * n);
    REFK_NEED(modulus, modulus_len, decomp_size);
    REFK_NEED(upper_half_increment, inc_len, decomp_size);
    REFK_CHECKED();
    threshold_kernel<<<dim3(gx, decomp_size, 1), 256, 0, st(stream)>>>(D(plain), out, M(modulus), D(upper_half_increment),
                                                                      upper_half_threshold, n_power, decomp_size);
    REFK_DONE();
}

/* cipherplain_kernel (multiplication.cu:298-311): cipher / output [2][decomp_size][n], plain [decomp_size][n].
 * Grid dim3(n >> 8, Q_size, 2), 256: bfv/operator.cu:441, 489. */
int refk_cipherplain(const uint64_t* cipher, i64 cipher_len, const uint64_t* plain, i64 plain_len, uint64_t* out,
                     i64 out_len, const void* modulus, i64 modulus_len, int n_power, int decomp_size, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(decomp_size);
    REFK_NEED(cipher, cipher_len, 2 * (i64) decomp_size * n);
    REFK_NEED(plain, plain_len, (i64) decomp_size * n);
    REFK_NEED(out, out_len, 2 * (i64) decomp_size * n);
    REFK_NEED(modulus, modulus_len, decomp_size);
    REFK_CHECKED();
    cipherplain_kernel<<<dim3(gx, decomp_size, 2), 256, 0, st(stream)>>>(D(cipher), D(plain), out, M(modulus), n_power,
                                                                        decomp_size);
    REFK_DONE();
}

/* cipher_mult_by_i_kernel / cipher_div_by_i_kernel (multiplication.cu:441-495): location < parts * limbs * n,
 * ntt_table[1 + (block_y << n_power)].  Grid dim3(n >> 8, current_decomp_count, cipher_size), 256:
 * ckks/operator.cu:759, 786. */
int refk_ckks_mult_i(int divide, const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, const uint64_t* ntt_table,
                     i64 table_len, const void* modulus, i64 modulus_len, int n_power, int limbs, int parts, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(limbs);
    REFK_COUNT(parts);
    const i64 words = (i64) parts * limbs * n;
    REFK_NEED(in, in_len, words);
    REFK_NEED(out, out_len, words);
    REFK_NEED(ntt_table, table_len, (i64) (limbs - 1) * n + 2);
    REFK_NEED(modulus, modulus_len, limbs);
    REFK_CHECKED();
    const dim3 grid(gx, limbs, parts);
    if (divide)
        cipher_div_by_i_kernel<<<grid, 256, 0, st(stream)>>>(D(in), out, D(ntt_table), M(modulus), n_power);
    else
        cipher_mult_by_i_kernel<<<grid, 256, 0, st(stream)>>>(D(in), out, D(ntt_table), M(modulus), n_power);
    REFK_DONE();
}

/* cipher_add_by_gaussian_integer_kernel / cipher_mult_by_gaussian_integer_kernel (multiplication.cu:497-570):
 * real_rns / imag_rns [block_y < limbs], ntt_table[1 + (block_y << n_power)].
 * Grid dim3(n >> 8, current_decomp_count, cipher_size), 256: ckks/operator.cu:622, 715. */
int refk_ckks_gaussian_integer_op(int op, const uint64_t* in, i64 in_len, const uint64_t* real_rns, i64 real_len,
                                  const uint64_t* imag_rns, i64 imag_len, uint64_t* out, i64 out_len,
                                  const uint64_t* ntt_table, i64 table_len, const void* modulus, i64 modulus_len,
                                  int n_power, int limbs, int parts, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(limbs);
    REFK_COUNT(parts);
    if (op < 0 || op > 1) return REFK_E_ARG;
    const i64 words = (i64) parts * limbs * n;
    REFK_NEED(in, in_len, words);
    REFK_NEED(real_rns, real_len, limbs);
    REFK_NEED(imag_rns, imag_len, limbs);
    REFK_NEED(out, out_len, words);
    REFK_NEED(ntt_table, table_len, (i64) (limbs - 1) * n + 2);
    REFK_NEED(modulus, modulus_len, limbs);
    REFK_CHECKED();
    const dim3 grid(gx, limbs, parts);
    if (op == 0)
        cipher_add_by_gaussian_integer_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(real_rns), D(imag_rns), out,
                                                                            D(ntt_table), M(modulus), n_power);
    else
        cipher_mult_by_gaussian_integer_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(real_rns), D(imag_rns), out,
                                                                             D(ntt_table), M(modulus), n_power);
    REFK_DONE();
}

/* ------------------------------------------------------------------ switchkey.cu: decomposition */
/* cipher_broadcast_kernel (switchkey.cu:11-27): input [grid.y][n], output [grid.y][rns_mod_count][n], modulus[i <
 * rns_mod_count].  Grid dim3(n >> 8, Q_size, 1), 256 with rns_mod_count = Q_prime_size: bfv/operator.cu:517. */
int refk_cipher_broadcast(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, const void* modulus,
                          i64 modulus_len, int n_power, int Q_size, int rns_mod_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(Q_size);
    REFK_COUNT(rns_mod_count);
    REFK_NEED(in, in_len, (i64) Q_size * n);
    REFK_NEED(out, out_len, (i64) Q_size * rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, rns_mod_count);
    REFK_CHECKED();
    cipher_broadcast_kernel<<<dim3(gx, Q_size, 1), 256, 0, st(stream)>>>(D(in), out, M(modulus), n_power, rns_mod_count);
    REFK_DONE();
}

/* cipher_broadcast_leveled_kernel (switchkey.cu:29-59): input [grid.y][n], output [grid.y][current_rns][n],
 * modulus[i < grid.y ? i : i + first_rns - current_rns] <= first_rns - 1.
 * Grid dim3(n >> 8, current_decomp_count, 1), 256: ckks/operator.cu:932. */
int refk_cipher_broadcast_leveled(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, const void* modulus,
                                  i64 modulus_len, int first_rns_mod_count, int current_rns_mod_count, int n_power,
                                  int current_decomp_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_count);
    REFK_COUNT(current_rns_mod_count);
    if (current_rns_mod_count > first_rns_mod_count || current_decomp_count > current_rns_mod_count) return REFK_E_ARG;
    REFK_NEED(in, in_len, (i64) current_decomp_count * n);
    REFK_NEED(out, out_len, (i64) current_decomp_count * current_rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, first_rns_mod_count);
    REFK_CHECKED();
    cipher_broadcast_leveled_kernel<<<dim3(gx, current_decomp_count, 1), 256, 0, st(stream)>>>(
        D(in), out, M(modulus), first_rns_mod_count, current_rns_mod_count, n_power);
    REFK_DONE();
}

/* cipher_broadcast_switchkey_leveled_kernel (switchkey.cu:1370-1411): cipher [2][l][n]; out0 [l][n] gets part 0, out1
 * [l][current_rns][n] part 1 reduced into every modulus (index <= first_rns - 1).
 * Grid dim3(n >> 8, current_decomp_count, 2), 256: ckks/operator.cu:1765. */
int refk_cipher_broadcast_switchkey_leveled(const uint64_t* cipher, i64 cipher_len, uint64_t* out0, i64 out0_len,
                                            uint64_t* out1, i64 out1_len, const void* modulus, i64 modulus_len,
                                            int n_power, int first_rns_mod_count, int current_rns_mod_count,
                                            int current_decomp_mod_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_mod_count);
    REFK_COUNT(current_rns_mod_count);
    if (current_rns_mod_count > first_rns_mod_count || current_decomp_mod_count > current_rns_mod_count) return REFK_E_ARG;
    REFK_NEED(cipher, cipher_len, 2 * (i64) current_decomp_mod_count * n);
    REFK_NEED(out0, out0_len, (i64) current_decomp_mod_count * n);
    REFK_NEED(out1, out1_len, (i64) current_decomp_mod_count * current_rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, first_rns_mod_count);
    REFK_CHECKED();
    cipher_broadcast_switchkey_leveled_kernel<<<dim3(gx, current_decomp_mod_count, 2), 256, 0, st(stream)>>>(
        D(cipher), out0, out1, M(modulus), n_power, first_rns_mod_count, current_rns_mod_count, current_decomp_mod_count);
    REFK_DONE();
}

/* ckks_duplicate_kernel (switchkey.cu:1558-1590): reads part 1 of cipher [2][l][n], output [l][current_rns][n].
 * Grid dim3(n >> 8, current_decomp_count, 1), 256: ckks/operator.cu:1467. */
int refk_ckks_duplicate(const uint64_t* cipher, i64 cipher_len, uint64_t* out, i64 out_len, const void* modulus,
                        i64 modulus_len, int n_power, int first_rns_mod_count, int current_rns_mod_count,
                        int current_decomp_mod_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_mod_count);
    REFK_COUNT(current_rns_mod_count);
    if (current_rns_mod_count > first_rns_mod_count || current_decomp_mod_count > current_rns_mod_count) return REFK_E_ARG;
    REFK_NEED(cipher, cipher_len, 2 * (i64) current_decomp_mod_count * n);
    REFK_NEED(out, out_len, (i64) current_decomp_mod_count * current_rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, first_rns_mod_count);
    REFK_CHECKED();
    ckks_duplicate_kernel<<<dim3(gx, current_decomp_mod_count, 1), 256, 0, st(stream)>>>(
        D(cipher), out, M(modulus), n_power, first_rns_mod_count, current_rns_mod_count, current_decomp_mod_count);
    REFK_DONE();
}

/* bfv_duplicate_kernel (switchkey.cu:1592-1619): cipher [2][Q][n], output1 [Q][n] (part 0), output2
 * [Q][rns_mod_count][n] (part 1 in every modulus).  Grid dim3(n >> 8, Q_size, 2), 256: bfv/operator.cu:791. */
int refk_bfv_duplicate(const uint64_t* cipher, i64 cipher_len, uint64_t* out1, i64 out1_len, uint64_t* out2, i64 out2_len,
                       const void* modulus, i64 modulus_len, int n_power, int Q_size, int rns_mod_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(Q_size);
    REFK_COUNT(rns_mod_count);
    REFK_NEED(cipher, cipher_len, 2 * (i64) Q_size * n);
    REFK_NEED(out1, out1_len, (i64) Q_size * n);
    REFK_NEED(out2, out2_len, (i64) Q_size * rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, rns_mod_count);
    REFK_CHECKED();
    bfv_duplicate_kernel<<<dim3(gx, Q_size, 2), 256, 0, st(stream)>>>(D(cipher), out1, out2, M(modulus), n_power,
                                                                     rns_mod_count);
    REFK_DONE();
}

/* base_conversion_DtoQtilde_relin_kernel (switchkey.cu:872-927, leveled == 0) and _leveled_kernel (:985-1046).
 * I_j / I_location are DEVICE int arrays [d]; h_I_j / h_I_location are the caller's HOST copies of the same values,
 * from which the ranges are checked (the kernels index the input, Mi_inv, the matrix and the moduli with them;
 * partial[] holds 20 words).  Output [d][Q_tilda][n].  Moduli: I_location + i < l, and i < Q_tilda (relin) or
 * i + level < Q_tilda + level (leveled).  mod_index is passed on; the kernel does not read it.
 * Grid dim3(n >> 8, d, 1), 256: bfv/operator.cu:600 (l = Q_size, Q_tilda = Q_prime_size); ckks/operator.cu:1066
 * (Q_tilda = current_rns_mod_count, l = current_decomp_count, level = depth). */
int refk_base_conversion_DtoQtilde(int leveled, const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len,
                                   const void* modulus, i64 modulus_len, const uint64_t* matrix, i64 matrix_len,
                                   const uint64_t* Mi_inv, i64 Mi_inv_len, const uint64_t* prod, i64 prod_len,
                                   const int* I_j, const int* I_location, i64 I_len, const int* h_I_j,
                                   const int* h_I_location, const int* mod_index, int n_power, int l, int Q_tilda, int d,
                                   int level, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(l);
    REFK_COUNT(Q_tilda);
    REFK_COUNT(d);
    if (level < 0 || (!leveled && level != 0)) return REFK_E_ARG;
    if (!h_I_j || !h_I_location) return REFK_E_NULL;
    REFK_NEED(I_j, I_len, d);
    REFK_NEED(I_location, I_len, d);
    i64 max_matrix = 0;
    for (int y = 0; y < d; y++) {
        const int cnt = h_I_j[y], at = h_I_location[y];
        if (cnt < 1 || cnt > 20 || at < 0) return REFK_E_ARG;
        if (at + cnt > l) return REFK_E_RANGE;
        const i64 end = (i64) at * Q_tilda + (i64) Q_tilda * cnt;
        if (end > max_matrix) max_matrix = end;
    }
    REFK_NEED(in, in_len, (i64) l * n);
    REFK_NEED(out, out_len, (i64) d * Q_tilda * n);
    REFK_NEED(modulus, modulus_len, (i64) Q_tilda + level > l ? (i64) Q_tilda + level : l);
    REFK_NEED(matrix, matrix_len, max_matrix);
    REFK_NEED(Mi_inv, Mi_inv_len, l);
    REFK_NEED(prod, prod_len, (i64) d * Q_tilda);
    REFK_CHECKED();
    if (leveled)
        base_conversion_DtoQtilde_relin_leveled_kernel<<<dim3(gx, d, 1), 256, 0, st(stream)>>>(
            D(in), out, M(modulus), D(matrix), D(Mi_inv), D(prod), (int*) I_j, (int*) I_location, n_power, d, Q_tilda, l,
            level, (int*) mod_index);
    else
        base_conversion_DtoQtilde_relin_kernel<<<dim3(gx, d, 1), 256, 0, st(stream)>>>(
            D(in), out, M(modulus), D(matrix), D(Mi_inv), D(prod), (int*) I_j, (int*) I_location, n_power, l, Q_tilda, d);
    REFK_DONE();
}

/* ------------------------------------------------------------------ switchkey.cu: inner product */
/* keyswitch_multiply_accumulate_kernel (switchkey.cu:61-162): input [digits][Qt][n], relinkey [digits][2][Qt][n],
 * output [2][Qt][n], modulus[block_y < Qt]; iteration_count1 = digits / 4, iteration_count2 = digits % 4.
 * Grid dim3(n >> 8, Q_prime_size, 1), 256: bfv/operator.cu:537-547. */
int refk_keyswitch_multiply_accumulate(const uint64_t* in, i64 in_len, const uint64_t* key, i64 key_len, uint64_t* out,
                                       i64 out_len, const void* modulus, i64 modulus_len, int n_power, int Q_tilda_size,
                                       int digits, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(Q_tilda_size);
    REFK_COUNT(digits);
    REFK_NEED(in, in_len, (i64) digits * Q_tilda_size * n);
    REFK_NEED(key, key_len, 2 * (i64) digits * Q_tilda_size * n);
    REFK_NEED(out, out_len, 2 * (i64) Q_tilda_size * n);
    REFK_NEED(modulus, modulus_len, Q_tilda_size);
    REFK_CHECKED();
    keyswitch_multiply_accumulate_kernel<<<dim3(gx, Q_tilda_size, 1), 256, 0, st(stream)>>>(
        D(in), key, out, M(modulus), n_power, Q_tilda_size, digits / 4, digits % 4);
    REFK_DONE();
}

/* keyswitch_multiply_accumulate_leveled_kernel (switchkey.cu:164-285): grid.y = l + 1 rows, row l is the special
 * prime (key / modulus index first_rns - 1); input [l][l + 1][n], relinkey [>= l][2][first_rns][n], output
 * [2][l + 1][n]; iteration counts from l.  Grid dim3(n >> 8, current_rns_mod_count, 1), 256 with
 * current_rns_mod_count = current_decomp_count + 1 (one special prime): ckks/operator.cu:963-972. */
int refk_keyswitch_multiply_accumulate_leveled(const uint64_t* in, i64 in_len, const uint64_t* key, i64 key_len,
                                               uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len,
                                               int first_rns_mod_count, int current_decomp_mod_count, int n_power,
                                               void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_mod_count);
    const int l = current_decomp_mod_count, rows = l + 1;
    if (rows > first_rns_mod_count) return REFK_E_ARG;
    REFK_NEED(in, in_len, (i64) l * rows * n);
    REFK_NEED(key, key_len, 2 * (i64) l * first_rns_mod_count * n);
    REFK_NEED(out, out_len, 2 * (i64) rows * n);
    REFK_NEED(modulus, modulus_len, first_rns_mod_count);
    REFK_CHECKED();
    keyswitch_multiply_accumulate_leveled_kernel<<<dim3(gx, rows, 1), 256, 0, st(stream)>>>(
        D(in), key, out, M(modulus), first_rns_mod_count, l, l / 4, l % 4, n_power);
    REFK_DONE();
}

/* keyswitch_multiply_accumulate_leveled_method_II_kernel (switchkey.cu:287-398): input [digits][current_rns][n],
 * relinkey [>= digits][2][first_rns][n] read at modulus index block_y (< l) or block_y + level, output
 * [2][current_rns][n].  Grid dim3(n >> 8, current_rns_mod_count, 1), 256, iteration counts from d_leveled[depth],
 * level = depth: ckks/operator.cu:1103-1115. */
int refk_keyswitch_multiply_accumulate_leveled_method_II(const uint64_t* in, i64 in_len, const uint64_t* key, i64 key_len,
                                                         uint64_t* out, i64 out_len, const void* modulus,
                                                         i64 modulus_len, int first_rns_mod_count,
                                                         int current_decomp_mod_count, int current_rns_mod_count,
                                                         int digits, int level, int n_power, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_mod_count);
    REFK_COUNT(current_rns_mod_count);
    REFK_COUNT(digits);
    if (level < 0 || current_rns_mod_count + level > first_rns_mod_count || current_decomp_mod_count > current_rns_mod_count)
        return REFK_E_ARG;
    REFK_NEED(in, in_len, (i64) digits * current_rns_mod_count * n);
    REFK_NEED(key, key_len, 2 * (i64) digits * first_rns_mod_count * n);
    REFK_NEED(out, out_len, 2 * (i64) current_rns_mod_count * n);
    REFK_NEED(modulus, modulus_len, first_rns_mod_count);
    REFK_CHECKED();
    keyswitch_multiply_accumulate_leveled_method_II_kernel<<<dim3(gx, current_rns_mod_count, 1), 256, 0, st(stream)>>>(
        D(in), key, out, M(modulus), first_rns_mod_count, current_decomp_mod_count, current_rns_mod_count, digits / 4,
        digits % 4, level, n_power);
    REFK_DONE();
}

/* ------------------------------------------------------------------ switchkey.cu: mod-down */
/* divide_round_lastq_kernel / _switchkey_kernel (switchkey.cu:400-478): input [2][Q + 1][n], ct / output [2][Q][n]
 * (the switchkey form reads ct for part 0 only), modulus[<= Q], half[0], half_mod / last_q_modinv [block_y < Q].
 * Grid dim3(n >> 8, Q_size, 2), 256: bfv/operator.cu:576, 1258. */
int refk_divide_round_lastq(int switchkey, const uint64_t* in, i64 in_len, const uint64_t* ct, i64 ct_len, uint64_t* out,
                            i64 out_len, const void* modulus, i64 modulus_len, const uint64_t* half, i64 half_len,
                            const uint64_t* half_mod, i64 half_mod_len, const uint64_t* last_q_modinv, i64 lqm_len,
                            int n_power, int decomp_mod_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(decomp_mod_count);
    const i64 Q = decomp_mod_count;
    REFK_NEED(in, in_len, 2 * (Q + 1) * n);
    REFK_NEED(ct, ct_len, (switchkey ? 1 : 2) * Q * n);
    REFK_NEED(out, out_len, 2 * Q * n);
    REFK_NEED(modulus, modulus_len, Q + 1);
    REFK_NEED(half, half_len, 1);
    REFK_NEED(half_mod, half_mod_len, Q);
    REFK_NEED(last_q_modinv, lqm_len, Q);
    REFK_CHECKED();
    const dim3 grid(gx, decomp_mod_count, 2);
    if (switchkey)
        divide_round_lastq_switchkey_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(ct), out, M(modulus), D(half),
                                                                          D(half_mod), D(last_q_modinv), n_power,
                                                                          decomp_mod_count);
    else
        divide_round_lastq_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(ct), out, M(modulus), D(half), D(half_mod),
                                                                D(last_q_modinv), n_power, decomp_mod_count);
    REFK_DONE();
}

/* the shared checks of the multi-prime mod-down kernels: input [2][Q_prime_size][n] with the P special limbs at
 * Q_size .. Q_size + P - 1, last_ct[15], modulus[first_Q_prime_size - 1 - i] and [first_Q_size + j], half[i < P],
 * half_mod / last_q_modinv walked by moddown_table_words() */
#define REFK_MODDOWN_CHECKS()                                                                                        \
    REFK_GEOMETRY(n_power);                                                                                          \
    REFK_COUNT(Q_size);                                                                                              \
    REFK_COUNT(P_size);                                                                                              \
    if (P_size > 15 || Q_size + P_size > Q_prime_size || first_Q_size + P_size > first_Q_prime_size ||               \
        Q_size > first_Q_size || Q_prime_size > first_Q_prime_size)                                                  \
        return REFK_E_ARG;                                                                                           \
    REFK_NEED(in, in_len, 2 * (i64) Q_prime_size * n);                                                               \
    REFK_NEED(out, out_len, 2 * (i64) Q_size * n);                                                                   \
    REFK_NEED(modulus, modulus_len, first_Q_prime_size);                                                             \
    REFK_NEED(half, half_len, P_size);                                                                               \
    REFK_NEED(half_mod, half_mod_len, moddown_table_words(first_Q_prime_size, P_size));                              \
    REFK_NEED(last_q_modinv, lqm_len, moddown_table_words(first_Q_prime_size, P_size))

/* divide_round_lastq_extended_leveled_kernel (mode 0, switchkey.cu:1222-1282, ckks/operator.cu:1136),
 * divide_round_lastq_extended_kernel (mode 1, :480-543, bfv/operator.cu:663) and _extended_switchkey_kernel (mode 2,
 * :545-611, bfv/operator.cu:1362).  Grid dim3(n >> 8, Q_size, 2), 256 at all three sites.  Modes 1 / 2 take the chain
 * sizes as their Q_prime_size / Q_size, so first_* must equal them; ct [2][Q][n] (mode 2 reads part 0 only). */
int refk_divide_round_lastq_extended(int mode, const uint64_t* in, i64 in_len, const uint64_t* ct, i64 ct_len,
                                     uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len,
                                     const uint64_t* half, i64 half_len, const uint64_t* half_mod, i64 half_mod_len,
                                     const uint64_t* last_q_modinv, i64 lqm_len, int n_power, int Q_prime_size, int Q_size,
                                     int first_Q_prime_size, int first_Q_size, int P_size, void* stream)
{
    REFK_MODDOWN_CHECKS();
    if (mode < 0 || mode > 2) return REFK_E_ARG;
    if (mode != 0) {
        if (Q_prime_size != first_Q_prime_size || Q_size != first_Q_size) return REFK_E_ARG;
        REFK_NEED(ct, ct_len, (mode == 1 ? 2 : 1) * (i64) Q_size * n);
    }
    REFK_CHECKED();
    const dim3 grid(gx, Q_size, 2);
    if (mode == 0)
        divide_round_lastq_extended_leveled_kernel<<<grid, 256, 0, st(stream)>>>(
            D(in), out, M(modulus), D(half), D(half_mod), D(last_q_modinv), n_power, Q_prime_size, Q_size,
            first_Q_prime_size, first_Q_size, P_size);
    else if (mode == 1)
        divide_round_lastq_extended_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(ct), out, M(modulus), D(half), D(half_mod),
                                                                         D(last_q_modinv), n_power, Q_prime_size, Q_size,
                                                                         P_size);
    else
        divide_round_lastq_extended_switchkey_kernel<<<grid, 256, 0, st(stream)>>>(
            D(in), D(ct), out, M(modulus), D(half), D(half_mod), D(last_q_modinv), n_power, Q_prime_size, Q_size, P_size);
    REFK_DONE();
}

/* divide_round_lastq_permute_ckks_kernel (bfv == 0, switchkey.cu:1621-1718, ckks/operator.cu:1530) and
 * divide_round_lastq_permute_bfv_kernel (bfv != 0, :1720-1813, bfv/operator.cu:854).  Grid dim3(n >> 8, Q_size, 2),
 * 256.  in2 [Q][n]; the store index is (idx * galois_elt) & (n - 1) in int arithmetic, so (n - 1) * galois_elt must
 * stay below 2^31. */
int refk_divide_round_lastq_permute(int bfv, const uint64_t* in, i64 in_len, const uint64_t* in2, i64 in2_len,
                                    uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len, const uint64_t* half,
                                    i64 half_len, const uint64_t* half_mod, i64 half_mod_len,
                                    const uint64_t* last_q_modinv, i64 lqm_len, int galois_elt, int n_power,
                                    int Q_prime_size, int Q_size, int first_Q_prime_size, int first_Q_size, int P_size,
                                    void* stream)
{
    REFK_MODDOWN_CHECKS();
    if (galois_elt < 1 || (galois_elt & 1) == 0 || (i64) galois_elt >= 2 * n || (n - 1) * (i64) galois_elt > 0x7fffffffLL)
        return REFK_E_ARG;
    if (bfv && (Q_prime_size != first_Q_prime_size || Q_size != first_Q_size)) return REFK_E_ARG;
    REFK_NEED(in2, in2_len, (i64) Q_size * n);
    REFK_CHECKED();
    const dim3 grid(gx, Q_size, 2);
    if (bfv)
        divide_round_lastq_permute_bfv_kernel<<<grid, 256, 0, st(stream)>>>(D(in), D(in2), out, M(modulus), D(half),
                                                                            D(half_mod), D(last_q_modinv), galois_elt,
                                                                            n_power, Q_prime_size, Q_size, P_size);
    else
        divide_round_lastq_permute_ckks_kernel<<<grid, 256, 0, st(stream)>>>(
            D(in), D(in2), out, M(modulus), D(half), D(half_mod), D(last_q_modinv), galois_elt, n_power, Q_prime_size,
            Q_size, first_Q_prime_size, first_Q_size, P_size);
    REFK_DONE();
}

/* divide_round_lastq_leveled_stage_one_kernel (switchkey.cu:678-705): input [2][cur + 1][n] (last limb at slot cur),
 * output [2][cur][n], modulus[first_decomp_count] and [i < cur], half[0], half_mod[i < cur].
 * Grid dim3(n >> 8, 2, 1), 256: ckks/operator.cu:1003 (relinearize) and :1205 (rescale, both counts l - 1). */
int refk_divide_round_lastq_leveled_stage_one(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len,
                                              const void* modulus, i64 modulus_len, const uint64_t* half, i64 half_len,
                                              const uint64_t* half_mod, i64 half_mod_len, int n_power,
                                              int first_decomp_count, int current_decomp_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_count);
    if (first_decomp_count < current_decomp_count) return REFK_E_ARG;
    const i64 cur = current_decomp_count;
    REFK_NEED(in, in_len, 2 * (cur + 1) * n);
    REFK_NEED(out, out_len, 2 * cur * n);
    REFK_NEED(modulus, modulus_len, (i64) first_decomp_count + 1);
    REFK_NEED(half, half_len, 1);
    REFK_NEED(half_mod, half_mod_len, cur);
    REFK_CHECKED();
    divide_round_lastq_leveled_stage_one_kernel<<<dim3(gx, 2, 1), 256, 0, st(stream)>>>(
        D(in), out, M(modulus), D(half), D(half_mod), n_power, first_decomp_count, current_decomp_count);
    REFK_DONE();
}

/* divide_round_lastq_leveled_stage_two_kernel / _switchkey_kernel (switchkey.cu:707-771): input_last / ct / output
 * [2][cur][n] (switchkey: ct part 0 only), input [2][cur + 1][n].
 * Grid dim3(n >> 8, current_decomp_count, 2), 256: ckks/operator.cu:1015, 1853. */
int refk_divide_round_lastq_leveled_stage_two(int switchkey, const uint64_t* in_last, i64 last_len, const uint64_t* in,
                                              i64 in_len, const uint64_t* ct, i64 ct_len, uint64_t* out, i64 out_len,
                                              const void* modulus, i64 modulus_len, const uint64_t* last_q_modinv,
                                              i64 lqm_len, int n_power, int current_decomp_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_count);
    const i64 cur = current_decomp_count;
    REFK_NEED(in_last, last_len, 2 * cur * n);
    REFK_NEED(in, in_len, (2 * cur + 1) * n);
    REFK_NEED(ct, ct_len, (switchkey ? 1 : 2) * cur * n);
    REFK_NEED(out, out_len, 2 * cur * n);
    REFK_NEED(modulus, modulus_len, cur);
    REFK_NEED(last_q_modinv, lqm_len, cur);
    REFK_CHECKED();
    const dim3 grid(gx, current_decomp_count, 2);
    if (switchkey)
        divide_round_lastq_leveled_stage_two_switchkey_kernel<<<grid, 256, 0, st(stream)>>>(
            D(in_last), D(in), D(ct), out, M(modulus), D(last_q_modinv), n_power, current_decomp_count);
    else
        divide_round_lastq_leveled_stage_two_kernel<<<grid, 256, 0, st(stream)>>>(
            D(in_last), D(in), D(ct), out, M(modulus), D(last_q_modinv), n_power, current_decomp_count);
    REFK_DONE();
}

/* move_cipher_leveled_kernel (switchkey.cu:776-790): limbs block_y < cur of both parts, part stride cur + 1 on both
 * sides: highest index (2 cur + 1) n - 1.  Grid dim3(n >> 8, current_decomp_count - 1, 2), 256 with the same count as
 * the argument: ckks/operator.cu:1219. */
int refk_move_cipher_leveled(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, int n_power,
                             int current_decomp_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_count);
    const i64 cur = current_decomp_count;
    REFK_NEED(in, in_len, (2 * cur + 1) * n);
    REFK_NEED(out, out_len, (2 * cur + 1) * n);
    REFK_CHECKED();
    move_cipher_leveled_kernel<<<dim3(gx, current_decomp_count, 2), 256, 0, st(stream)>>>(D(in), out, n_power,
                                                                                         current_decomp_count);
    REFK_DONE();
}

/* divide_round_lastq_rescale_kernel (switchkey.cu:792-815): input_last / output [2][cur][n], input part stride
 * cur + 1.  Grid dim3(n >> 8, current_decomp_count - 1, 2), 256: ckks/operator.cu:1225. */
int refk_divide_round_lastq_rescale(const uint64_t* in_last, i64 last_len, const uint64_t* in, i64 in_len, uint64_t* out,
                                    i64 out_len, const void* modulus, i64 modulus_len, const uint64_t* last_q_modinv,
                                    i64 lqm_len, int n_power, int current_decomp_count, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(current_decomp_count);
    const i64 cur = current_decomp_count;
    REFK_NEED(in_last, last_len, 2 * cur * n);
    REFK_NEED(in, in_len, (2 * cur + 1) * n);
    REFK_NEED(out, out_len, 2 * cur * n);
    REFK_NEED(modulus, modulus_len, cur);
    REFK_NEED(last_q_modinv, lqm_len, cur);
    REFK_CHECKED();
    divide_round_lastq_rescale_kernel<<<dim3(gx, current_decomp_count, 2), 256, 0, st(stream)>>>(
        D(in_last), D(in), out, M(modulus), D(last_q_modinv), n_power, current_decomp_count);
    REFK_DONE();
}

/* negacyclic_shift_poly_coeffmod_kernel (switchkey.cu:1433-1457): [parts][limbs][n] both sides, the store index is
 * (idx + shift) & (n - 1); the kernel scatters, so out must not be in.
 * Grid dim3(n >> 8, Q_size, 2), 256: bfv/operator.cu:1383 (`parts` here for the 2). */
int refk_negacyclic_shift(const uint64_t* in, i64 in_len, uint64_t* out, i64 out_len, const void* modulus, i64 modulus_len,
                          int shift, int n_power, int limbs, int parts, void* stream)
{
    REFK_GEOMETRY(n_power);
    REFK_COUNT(limbs);
    REFK_COUNT(parts);
    if (shift < 0 || (i64) shift >= 2 * n || in == out) return REFK_E_ARG;
    const i64 words = (i64) parts * limbs * n;
    REFK_NEED(in, in_len, words);
    REFK_NEED(out, out_len, words);
    REFK_NEED(modulus, modulus_len, limbs);
    REFK_CHECKED();
    negacyclic_shift_poly_coeffmod_kernel<<<dim3(gx, limbs, parts), 256, 0, st(stream)>>>(D(in), out, M(modulus), shift,
                                                                                         n_power);
    REFK_DONE();
}

} /* extern "C" */
