// keygen.hip -- key generation / encryption / decryption kernels for gfx950
// (SURVEY.md 8f next-1).  All of them are element-wise streams over
// [poly][limb][N] arrays (HBM-bound); the transforms between them are the NTT
// kernels of the hot path.
#include "keygen.hpp"
#include "crt_compose.cuh"
#include "ckks_const.cuh"

namespace hegpu {

#define KG_THREADS 256

__global__ __launch_bounds__(KG_THREADS) void k_kg_uniform(u64* __restrict__ out, const Mod* __restrict__ mods,
                                                           int n_power, int limbs, DrbgKey seed, u64 stream)
{
    const u64 n = (u64) blockIdx.x * KG_THREADS + threadIdx.x;
    const int limb = blockIdx.y, poly = blockIdx.z;
    const u64 e = (((u64) poly * limbs + limb) << n_power) + n;
    out[e] = drbg_uniform(seed, stream, e, mods[limb]);
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_gaussian(u64* __restrict__ out, const Mod* __restrict__ mods,
                                                            int n_power, int limbs, DrbgKey seed, u64 stream,
                                                            GaussCdt cdt)
{
    const u64 n = (u64) blockIdx.x * KG_THREADS + threadIdx.x;
    const int poly = blockIdx.y;
    const int v = drbg_gaussian(seed, stream, ((u64) poly << n_power) + n, cdt);
    for (int j = 0; j < limbs; j++) out[(((u64) poly * limbs + j) << n_power) + n] = lift_small(v, mods[j].q);
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_ternary(u64* __restrict__ out, const Mod* __restrict__ mods,
                                                           int n_power, int limbs, DrbgKey seed, u64 stream)
{
    const u64 n = (u64) blockIdx.x * KG_THREADS + threadIdx.x;
    const int poly = blockIdx.y;
    const int v = drbg_ternary(seed, stream, ((u64) poly << n_power) + n);
    for (int j = 0; j < limbs; j++) out[(((u64) poly * limbs + j) << n_power) + n] = lift_small(v, mods[j].q);
}

hipError_t kg_uniform(u64* out, const Mod* mods, int n_power, int limbs, int polys, DrbgKey seed, u64 stream,
                      hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_uniform, dim3((1u << n_power) / KG_THREADS, limbs, polys), dim3(KG_THREADS), 0, st, out,
                       mods, n_power, limbs, seed, stream);
    return hipGetLastError();
}
hipError_t kg_gaussian(u64* out, const Mod* mods, int n_power, int limbs, int polys, DrbgKey seed, u64 stream,
                       const GaussCdt& cdt, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_gaussian, dim3((1u << n_power) / KG_THREADS, polys), dim3(KG_THREADS), 0, st, out, mods,
                       n_power, limbs, seed, stream, cdt);
    return hipGetLastError();
}
hipError_t kg_ternary(u64* out, const Mod* mods, int n_power, int limbs, int polys, DrbgKey seed, u64 stream,
                      hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_ternary, dim3((1u << n_power) / KG_THREADS, polys), dim3(KG_THREADS), 0, st, out, mods,
                       n_power, limbs, seed, stream);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_secret_rns(const int* __restrict__ positions,
                                                              const int* __restrict__ values, int count,
                                                              u64* __restrict__ out, const Mod* __restrict__ mods,
                                                              int n_power, int limbs)
{
    const int i = blockIdx.x * KG_THREADS + threadIdx.x;
    if (i >= count) return;
    const int pos = positions[i], v = values[i];
    for (int j = 0; j < limbs; j++) out[((u64) j << n_power) + pos] = lift_small(v, mods[j].q);
}

hipError_t kg_secret_rns(const int* positions, const int* values, int count, u64* out, const Mod* mods, int n_power,
                         int limbs, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(out, 0, ((size_t) limbs << n_power) * sizeof(u64), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_kg_secret_rns, dim3((count + KG_THREADS - 1) / KG_THREADS), dim3(KG_THREADS), 0, st,
                       positions, values, count, out, mods, n_power, limbs);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_publickey(u64* __restrict__ pk, const u64* __restrict__ sk,
                                                             const u64* __restrict__ e, const u64* __restrict__ a,
                                                             const Mod* __restrict__ mods, int n_power, int limbs)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    const Mod m = mods[blockIdx.y];
    const u64 av = a[loc];
    u64 t = mul_barrett(sk[loc], av, m);
    t = add_mod(t, e[loc], m.q);
    pk[loc] = sub_mod(0, t, m.q);
    pk[loc + ((u64) limbs << n_power)] = av;
}

hipError_t kg_publickey(u64* pk, const u64* sk, const u64* e, const u64* a, const Mod* mods, int n_power, int limbs,
                        hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_publickey, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, pk, sk, e,
                       a, mods, n_power, limbs);
    return hipGetLastError();
}

__device__ __forceinline__ u32 bitrev(u32 v, int bits) { return __brev(v) >> (32 - bits); }

// slot permutation of an NTT-domain polynomial under X -> X^g (keygeneration.cu:742-755)
__device__ __forceinline__ u32 ntt_permutation(u32 index, u32 galois_elt, int n_power)
{
    const u32 n = 1u << n_power;
    const u32 reversed = bitrev(index + n, n_power + 1);
    const u32 raw = ((galois_elt * reversed) >> 1) & (n - 1);
    return bitrev(raw, n_power);
}

// One kernel for the six generators of the reference (keygeneration.cu relinkey_gen_kernel :145,
// relinkey_gen_II_kernel :584, galoiskey_gen_kernel :757, galoiskey_gen_II_kernel :807,
// switchkey_gen_kernel :896, switchkey_gen_II_kernel :941).  Digit i of the key is
//   ( -(s' * a_i + e_i) + [limb y belongs to digit i] * carried * P  ,  a_i )   over the Q' limbs,
// with (s', carried) = (s, s^2) relinearisation, (s o g^-1, s) Galois, (s_new, s_old) switch key.
// Method I: digits = Q, digit_width = 1, P = the one special prime; method II: digits of
// digit_width primes (Sk_pair = y / width; special limbs belong to no digit), P = product of the
// special primes, multiplied in one factor at a time like the reference.
// With u != nullptr the same body writes a party's round-1 share of the collective relinearisation key
// (multi_party_relinkey_piece_method_I / _II_stage_I_kernel :190-278):
//   ( -(u * a_i) + e_i + [limb y belongs to digit i] * s * P  ,  s * a_i + e1_i ),
// u the party's ephemeral ternary secret (NTT domain), a_i the parties' common randomness.
__global__ __launch_bounds__(KG_THREADS) void k_kg_switchkey(u64* __restrict__ key, const u64* __restrict__ sk,
                                                             const u64* __restrict__ e, const u64* __restrict__ a,
                                                             const Mod* __restrict__ mods,
                                                             const u64* __restrict__ factor, int galois_elt,
                                                             const u64* __restrict__ old_sk,
                                                             const u64* __restrict__ u, const u64* __restrict__ e1,
                                                             int n_power, int limbs, int digits, int digit_width,
                                                             int q_size, int p_size)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const int y = blockIdx.y;
    const Mod m = mods[y];
    const u64 s = sk[idx + ((u64) y << n_power)];
    const u64 sp = u ? u[idx + ((u64) y << n_power)]
                     : galois_elt ? sk[((u64) y << n_power) + ntt_permutation(idx, (u32) galois_elt, n_power)] : s;
    u64 carried = old_sk ? old_sk[idx + ((u64) y << n_power)] : ((galois_elt || u) ? s : mul_barrett(s, s, m));
    const int own = (y < q_size) ? y / digit_width : -1;
    if (own >= 0)
        for (int j = 0; j < p_size; j++) carried = mul_barrett(carried, factor[j * q_size + y], m);
    for (int i = 0; i < digits; i++) {
        const u64 src = idx + ((u64) y << n_power) + ((u64) (limbs * i) << n_power);
        const u64 av = a[src];
        u64 k0 = mul_barrett(sp, av, m);
        if (u) { // round 1: the error is added to -(u * a), not negated with it (:210-212)
            k0 = sub_mod(0, k0, m.q);
            k0 = add_mod(k0, e[src], m.q);
        } else {
            k0 = add_mod(k0, e[src], m.q);
            k0 = sub_mod(0, k0, m.q);
        }
        if (i == own) k0 = add_mod(k0, carried, m.q);
        const u64 dst = idx + ((u64) y << n_power) + ((u64) (limbs * i) << (n_power + 1));
        key[dst] = k0;
        key[dst + ((u64) limbs << n_power)] = u ? add_mod(mul_barrett(av, s, m), e1[src], m.q) : av;
    }
}

hipError_t kg_switchkey(u64* key, const u64* sk, const u64* e, const u64* a, const Mod* mods, const u64* factor,
                        int galois_elt, const u64* old_sk, int n_power, int limbs, int digits, int digit_width,
                        int q_size, int p_size, hipStream_t st, const u64* u, const u64* e1)
{
    hipLaunchKernelGGL(k_kg_switchkey, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, key, sk, e,
                       a, mods, factor, galois_elt, old_sk, u, e1, n_power, limbs, digits, digit_width, q_size, p_size);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_pk_u(const u64* __restrict__ pk, const u64* __restrict__ u,
                                                        u64* __restrict__ out, const Mod* __restrict__ mods,
                                                        int n_power, int limbs)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    const u64 z = ((u64) limbs << n_power) * blockIdx.z;
    out[loc + z] = mul_barrett(pk[loc + z], u[loc], mods[blockIdx.y]);
}

hipError_t kg_pk_u(const u64* pk, const u64* u, u64* out, const Mod* mods, int n_power, int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_pk_u, dim3((1u << n_power) / KG_THREADS, limbs, 2), dim3(KG_THREADS), 0, st, pk, u, out,
                       mods, n_power, limbs);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_message_add(u64* __restrict__ ct, const u64* __restrict__ plain,
                                                               const Mod* __restrict__ mods, int n_power)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    ct[loc] = add_mod(ct[loc], plain[loc], mods[blockIdx.y].q);
}

hipError_t kg_message_add(u64* ct, const u64* plain, const Mod* mods, int n_power, int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_message_add, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, ct, plain,
                       mods, n_power);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_sk_mul_ckks(const u64* __restrict__ ct, u64* __restrict__ plain,
                                                               const u64* __restrict__ sk,
                                                               const Mod* __restrict__ mods, int n_power, int limbs)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    const Mod m = mods[blockIdx.y];
    const u64 c1 = mul_barrett(ct[loc + ((u64) limbs << n_power)], sk[loc], m);
    plain[loc] = add_mod(c1, ct[loc], m.q);
}

hipError_t kg_sk_multiplication_ckks(const u64* ct, u64* plain, const u64* sk, const Mod* mods, int n_power,
                                     int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_sk_mul_ckks, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, ct, plain,
                       sk, mods, n_power, limbs);
    return hipGetLastError();
}

// D(m), the scaled plaintext: bfv_scaled_plain of bfv_plain.cuh (shared with rns.hip k_gate_combine)
__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_message_add(u64* __restrict__ ct, const u64* __restrict__ plain,
                                                                   const Mod* __restrict__ mods,
                                                                   const u64* __restrict__ coeff_div, BfvPlainScale p,
                                                                   int n_power)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const int y = blockIdx.y;
    const Mod m = mods[y];
    const u64 loc = idx + ((u64) y << n_power);
    ct[loc] = add_mod(ct[loc], bfv_scaled_plain(plain[idx], m, coeff_div[y], p), m.q);
}

hipError_t kg_bfv_message_add(u64* ct, const u64* plain, const Mod* mods, const u64* coeff_div, const BfvPlainScale& p,
                              int n_power, int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_message_add, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, ct,
                       plain, mods, coeff_div, p, n_power);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_plain_addsub(const u64* __restrict__ ct,
                                                                    const u64* __restrict__ plain, u64* __restrict__ out,
                                                                    const Mod* __restrict__ mods,
                                                                    const u64* __restrict__ coeff_div, BfvPlainScale p,
                                                                    int n_power, int limbs, int sub)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    const Mod m = mods[y];
    const u64 loc = idx + ((u64) y << n_power) + (((u64) limbs * z) << n_power);
    u64 c = ct[loc];
    if (z == 0) {
        const u64 r = bfv_scaled_plain(plain[idx], m, coeff_div[y], p);
        c = sub ? sub_mod(c, r, m.q) : add_mod(r, c, m.q);
    }
    out[loc] = c;
}

hipError_t kg_bfv_plain_addsub(const u64* ct, const u64* plain, u64* out, const Mod* mods, const u64* coeff_div,
                               const BfvPlainScale& p, int n_power, int limbs, int sub, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_plain_addsub, dim3((1u << n_power) / KG_THREADS, limbs, 2), dim3(KG_THREADS), 0, st,
                       ct, plain, out, mods, coeff_div, p, n_power, limbs, sub);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_threshold(const u64* __restrict__ plain, u64* __restrict__ out,
                                                                 const Mod* __restrict__ mods,
                                                                 const u64* __restrict__ inc, u64 upper_threshold,
                                                                 int n_power)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const int y = blockIdx.y;
    const u64 v = plain[idx];
    out[idx + ((u64) y << n_power)] = (v >= upper_threshold) ? add_mod(v, inc[y], mods[y].q) : v;
}

hipError_t kg_bfv_threshold(const u64* plain, u64* out, const Mod* mods, const u64* upper_half_increment,
                            u64 upper_threshold, int n_power, int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_threshold, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, plain,
                       out, mods, upper_half_increment, upper_threshold, n_power);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_sk_mul(const u64* __restrict__ in, const u64* __restrict__ sk,
                                                          u64* __restrict__ out, const Mod* __restrict__ mods,
                                                          int n_power)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    out[loc] = mul_barrett(in[loc], sk[loc], mods[blockIdx.y]);
}

hipError_t kg_sk_multiplication(const u64* in, const u64* sk, u64* out, const Mod* mods, int n_power, int limbs,
                                hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_sk_mul, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, in, sk, out,
                       mods, n_power);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_coeff_multadd(const u64* __restrict__ ct0, const u64* __restrict__ x,
                                                                 u64* __restrict__ out, u64 t,
                                                                 const Mod* __restrict__ mods, int n_power)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power);
    const Mod m = mods[blockIdx.y];
    out[loc] = mul_barrett(add_mod(ct0[loc], x[loc], m.q), reduce64(t, m), m);
}

hipError_t kg_coeff_multadd(const u64* ct0, const u64* x, u64* out, u64 t, const Mod* mods, int n_power, int limbs,
                            hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_coeff_multadd, dim3((1u << n_power) / KG_THREADS, limbs), dim3(KG_THREADS), 0, st, ct0, x,
                       out, t, mods, n_power);
    return hipGetLastError();
}

// decryption_kernel (decryption.cu:44-120) in two steps: one limb of c0 + c1*s folded into the sums mod t and
// mod gamma, then the scale-and-round from the two sums
__device__ __forceinline__ void bfv_round_limb(u64 mt, int i, const Mod& m, const BfvDecryptDev& d, u64& sum_t,
                                               u64& sum_g)
{
    const u64 t = d.plain.q, g = d.gamma.q;
    const u64 g_i = reduce64(g, m);
    mt = mul_barrett(mt, t, m);
    mt = mul_barrett(mt, g_i, m);
    mt = mul_barrett(mt, d.Qi_inverse[i], m);
    u64 in_t = reduce64(mt, d.plain), in_g = reduce64(mt, d.gamma);
    in_t = mul_barrett(in_t, d.Qi_t[i], d.plain);
    in_g = mul_barrett(in_g, d.Qi_gamma[i], d.gamma);
    sum_t = add_mod(sum_t, in_t, t);
    sum_g = add_mod(sum_g, in_g, g);
}
__device__ __forceinline__ u64 bfv_round_finish(u64 sum_t, u64 sum_g, const BfvDecryptDev& d)
{
    const u64 t = d.plain.q, g = d.gamma.q;
    sum_t = mul_barrett(sum_t, d.mulq_inv_t, d.plain);
    sum_g = mul_barrett(sum_g, d.mulq_inv_gamma, d.gamma);
    u64 result;
    if (sum_g > (g >> 1)) {
        const u64 g_t = reduce64(g, d.plain), sg_t = reduce64(sum_g, d.plain);
        result = sub_mod(g_t, sg_t, t);
        result = add_mod(sum_t, result, t);
        result = mul_barrett(result, d.inv_gamma, d.plain);
    } else {
        const u64 st = reduce64(sum_t, d.plain), sg_t = reduce64(sum_g, d.plain);
        result = sub_mod(st, sg_t, t);
        result = mul_barrett(result, d.inv_gamma, d.plain);
    }
    return result;
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_decryption(const u64* __restrict__ ct0,
                                                                  const u64* __restrict__ ct1,
                                                                  u64* __restrict__ plain,
                                                                  const Mod* __restrict__ mods, BfvDecryptDev d,
                                                                  int n_power, int limbs)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    u64 sum_t = 0, sum_g = 0;
    for (int i = 0; i < limbs; i++) {
        const Mod m = mods[i];
        const u64 loc = idx + ((u64) i << n_power);
        bfv_round_limb(add_mod(ct0[loc], ct1[loc], m.q), i, m, d, sum_t, sum_g);
    }
    plain[idx] = bfv_round_finish(sum_t, sum_g, d);
}

hipError_t kg_bfv_decryption(const u64* ct0, const u64* ct1s, u64* plain, const Mod* mods, const BfvDecryptDev& d,
                             int n_power, int limbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_decryption, dim3((1u << n_power) / KG_THREADS), dim3(KG_THREADS), 0, st, ct0, ct1s,
                       plain, mods, d, n_power, limbs);
    return hipGetLastError();
}

__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_encode(u64* __restrict__ out,
                                                              const long long* __restrict__ message,
                                                              const int* __restrict__ location, u64 t,
                                                              int message_size)
{
    const int idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const int loc = location[idx];
    u64 v = 0;
    if (idx < message_size) {
        long long m = message[idx];
        if (m < 0) m += (long long) t;
        v = (u64) m;
    }
    out[loc] = v;
}
__global__ __launch_bounds__(KG_THREADS) void k_kg_bfv_decode(u64* __restrict__ message, const u64* __restrict__ in,
                                                              const int* __restrict__ location)
{
    const int idx = blockIdx.x * KG_THREADS + threadIdx.x;
    message[idx] = in[location[idx]];
}

hipError_t kg_bfv_encode_scatter(u64* out, const long long* message, const int* location, u64 t, int message_size,
                                 int n_power, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_encode, dim3((1u << n_power) / KG_THREADS), dim3(KG_THREADS), 0, st, out, message,
                       location, t, message_size);
    return hipGetLastError();
}
hipError_t kg_bfv_decode_gather(u64* message, const u64* in, const int* location, int n_power, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_bfv_decode, dim3((1u << n_power) / KG_THREADS), dim3(KG_THREADS), 0, st, message, in,
                       location);
    return hipGetLastError();
}

// ---- CKKS ciphertext (+,-,*) one real constant, and multiplication / division by the imaginary unit
// addition_constant_plain_ckks_poly / substraction_constant_plain_ckks_poly (addition.cu:219-300): part 0
// gets +-round(value) mod q_j, the other parts are copied; cipher_constant_plain_multiplication_kernel
// (multiplication.cu:333-372): every part times round(value) mod q_j.  |value| < 2^128.
__global__ __launch_bounds__(KG_THREADS) void k_kg_ckks_constant(const u64* __restrict__ ct, double value,
                                                                 u64* __restrict__ out, const Mod* __restrict__ mods,
                                                                 int n_power, int op)
{
    const u64 loc = (u64) blockIdx.x * KG_THREADS + threadIdx.x + ((u64) blockIdx.y << n_power) +
                    (((u64) gridDim.y * blockIdx.z) << n_power);
    const u64 x = ct[loc];
    if (op != 2 && blockIdx.z != 0) { out[loc] = x; return; }
    const Mod m = mods[blockIdx.y];
    const u64 pt = real_constant_residue(value, m);
    out[loc] = op == 0 ? add_mod(x, pt, m.q) : op == 1 ? sub_mod(x, pt, m.q) : mul_barrett(x, pt, m);
}

hipError_t kg_ckks_constant(const u64* ct, double value, u64* out, const Mod* mods, int n_power, int limbs, int parts,
                            int op, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_ckks_constant, dim3((1u << n_power) / KG_THREADS, limbs, parts), dim3(KG_THREADS), 0, st,
                       ct, value, out, mods, n_power, op);
    return hipGetLastError();
}

// cipher_add_by_gaussian_integer_kernel / cipher_mult_by_gaussian_integer_kernel (multiplication.cu:497-570):
// the constant round(re) + round(im) * i in every slot.  In the NTT domain i is +psi^(N/2) on the first half
// of the positions and -psi^(N/2) on the second, so the slot constant is re +- im * psi^(N/2) mod q_j; op 0
// adds it to part 0 (the other parts are copied), op 1 multiplies every part by it.  The reference turns the
// rounded doubles into residues with NTL big integers (ckks/operator.cu:583-617) and accepts any magnitude; a
// double is mant * 2^e: below 2^128 the residue comes from its two 64-bit halves, beyond that from
// (mant mod q) * (2^e mod q) -- exact for every finite double.
__global__ __launch_bounds__(KG_THREADS) void k_kg_ckks_gaussian(const u64* __restrict__ ct, double re, double im,
                                                                 u64* __restrict__ out, const u64* __restrict__ psi_half,
                                                                 const Mod* __restrict__ mods, int n_power, int op)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const u64 loc = idx + ((u64) blockIdx.y << n_power) + (((u64) gridDim.y * blockIdx.z) << n_power);
    const u64 x = ct[loc];
    if (op == 0 && blockIdx.z != 0) { out[loc] = x; return; }
    const Mod m = mods[blockIdx.y];
    const u64 k = gaussian_slot_constant(re, im, psi_half[blockIdx.y], idx < (1u << (n_power - 1)), m);
    out[loc] = op == 0 ? add_mod(x, k, m.q) : mul_barrett(x, k, m);
}

hipError_t kg_ckks_gaussian(const u64* ct, double re, double im, u64* out, const u64* psi_half, const Mod* mods,
                            int n_power, int limbs, int parts, int op, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_ckks_gaussian, dim3((1u << n_power) / KG_THREADS, limbs, parts), dim3(KG_THREADS), 0, st, ct,
                       re, im, out, psi_half, mods, n_power, op);
    return hipGetLastError();
}

// cipher_mult_by_i_kernel / cipher_div_by_i_kernel (multiplication.cu:441-495): in the NTT domain the
// monomial X^(N/2) (= i in every slot) is +psi^(N/2) on the first half of the positions and -psi^(N/2) on
// the second; psi_half[j] = forward table entry 1 of modulus j
__global__ __launch_bounds__(KG_THREADS) void k_kg_ckks_mult_i(const u64* __restrict__ ct, u64* __restrict__ out,
                                                               const u64* __restrict__ psi_half,
                                                               const Mod* __restrict__ mods, int n_power, int divide)
{
    const u32 idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const u64 loc = idx + ((u64) blockIdx.y << n_power) + (((u64) gridDim.y * blockIdx.z) << n_power);
    const Mod m = mods[blockIdx.y];
    const u64 psi = psi_half[blockIdx.y];
    const bool first = idx < (1u << (n_power - 1));
    const u64 w = (first != (divide != 0)) ? psi : sub_mod(0, psi, m.q);
    out[loc] = mul_barrett(ct[loc], w, m);
}

hipError_t kg_ckks_mult_i(const u64* ct, u64* out, const u64* psi_half, const Mod* mods, int n_power, int limbs,
                          int parts, int divide, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_ckks_mult_i, dim3((1u << n_power) / KG_THREADS, limbs, parts), dim3(KG_THREADS), 0, st, ct,
                       out, psi_half, mods, n_power, divide);
    return hipGetLastError();
}

// negacyclic_shift_poly_coeffmod_kernel (switchkey.cu:1433-1457): multiplication by X^shift in the coefficient
// domain; the wrapped coefficients are stored as q - x without a zero test, as the reference does
__global__ __launch_bounds__(KG_THREADS) void k_kg_negacyclic_shift(const u64* __restrict__ in, u64* __restrict__ out,
                                                                    const Mod* __restrict__ mods, int shift,
                                                                    int n_power)
{
    const int idx = blockIdx.x * KG_THREADS + threadIdx.x;
    const u64 base = ((u64) blockIdx.y << n_power) + (((u64) gridDim.y << n_power) * blockIdx.z);
    const int raw = idx + shift;
    u64 v = in[idx + base];
    if ((raw >> n_power) & 1) v = mods[blockIdx.y].q - v;
    out[(raw & ((1 << n_power) - 1)) + base] = v;
}

hipError_t kg_negacyclic_shift(const u64* in, u64* out, const Mod* mods, int shift, int n_power, int limbs, int parts,
                               hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_negacyclic_shift, dim3((1u << n_power) / KG_THREADS, limbs, parts), dim3(KG_THREADS), 0, st,
                       in, out, mods, shift, n_power);
    return hipGetLastError();
}

// ---- N-out-of-N multiparty protocol (host/{ckks,bfv}/mpcmanager.cu; keygeneration.cu:118-462, 861-894).
// The public-key and Galois-key shares are k_kg_publickey / k_kg_switchkey with the parties' common `a`, the round-1
// relinearisation share is k_kg_switchkey with u; what follows is the round-2 share, the k-way sums and the kernels of
// collective decryption, which the collective refresh below uses too: its share is the decryption share with a second
// half, its sums read one half of a share.  All of them are HBM streams: two coefficients (16 bytes) per lane per array.
#define KG_VEC 2
typedef ulonglong2 u64x2;

__device__ __forceinline__ u64x2 ld2(const u64* p) { return *reinterpret_cast<const u64x2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64x2 v) { *reinterpret_cast<u64x2*>(p) = v; }
__device__ __forceinline__ u64x2 add2(u64x2 a, u64x2 b, u64 q) { return u64x2{add_mod(a.x, b.x, q), add_mod(a.y, b.y, q)}; }
__device__ __forceinline__ u64x2 sub2(u64x2 a, u64x2 b, u64 q) { return u64x2{sub_mod(a.x, b.x, q), sub_mod(a.y, b.y, q)}; }
__device__ __forceinline__ u64x2 mul2(u64x2 a, u64x2 b, const Mod& m)
{
    return u64x2{mul_barrett(a.x, b.x, m), mul_barrett(a.y, b.y, m)};
}
static inline dim3 vec_grid(int n_power, int y, int z) { return dim3((1u << n_power) / (KG_THREADS * KG_VEC), y, z); }

// multi_party_relinkey_piece_method_I_II_stage_II_kernel (:280-319): from the summed round-1 shares (h0_d, h1_d)
//   share_d = ( s * h0_d + e2_d ,  (u - s) * h1_d + e3_d );   e = [2][digits][limbs][N], e2 first
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_relin_round2(u64* __restrict__ share, const u64* __restrict__ h,
                                                                    const u64* __restrict__ sk, const u64* __restrict__ u,
                                                                    const u64* __restrict__ e,
                                                                    const Mod* __restrict__ mods, int n_power, int limbs)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int y = blockIdx.y, i = blockIdx.z, digits = gridDim.z;
    const Mod m = mods[y];
    const u64 lane = n + ((u64) y << n_power);
    const u64x2 s = ld2(sk + lane), us = sub2(ld2(u + lane), s, m.q);
    const u64 key = lane + ((u64) (limbs * i) << (n_power + 1)), part = (u64) limbs << n_power;
    const u64 err = lane + ((u64) (limbs * i) << n_power);
    st2(share + key, add2(mul2(ld2(h + key), s, m), ld2(e + err), m.q));
    st2(share + key + part, add2(mul2(ld2(h + key + part), us, m), ld2(e + err + (part * digits)), m.q));
}

hipError_t kg_mpc_relin_round2(u64* share, const u64* round1_sum, const u64* sk, const u64* u, const u64* e,
                               const Mod* mods, int n_power, int limbs, int digits, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_mpc_relin_round2, vec_grid(n_power, limbs, digits), dim3(KG_THREADS), 0, st, share,
                       round1_sum, sk, u, e, mods, n_power, limbs);
    return hipGetLastError();
}

// The share pointers (a HOST array of k device pointers) reach the kernels KG_MPC_MAX_SHARES at a time:
// launch(group, count, first) once per group, in order.  What a later group reads as its base is the caller's rule.
template <class F> static hipError_t each_share_group(const u64* const* shares, int k, F&& launch)
{
    for (int done = 0; done < k; done += KG_MPC_MAX_SHARES) {
        MpcShares sh{};
        const int cnt = k - done < KG_MPC_MAX_SHARES ? k - done : KG_MPC_MAX_SHARES;
        for (int j = 0; j < cnt; j++) sh.p[j] = shares[done + j];
        launch(sh, cnt, done == 0);
    }
    return hipGetLastError();
}

// threshold_pk_addition (:118-140), multi_party_relinkey_method_I_stage_I / _II_kernel (:321-462),
// multi_party_galoiskey_method_I_II_kernel (:861-894): the reference adds one share per launch; here one launch reads
// each of k <= KG_MPC_MAX_SHARES shares once and writes the sum once.  A unit (blockIdx.z) is [2][limbs][N]: the public
// key, or one digit of a switching key.  Part 0 = carry + sum of the shares' parts 0 (fold: parts 0 and 1, the last
// step of the relinearisation key); part 1 = carry + sum of the parts 1 (sum_second), a copy of `second`'s part 1
// (second != nullptr), or left alone.  carry (may be `out`): the sum of an earlier group of shares.
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_accumulate(u64* out, MpcShares sh, int k, const u64* carry,
                                                                  const u64* second, int fold, int sum_second,
                                                                  const Mod* __restrict__ mods, int n_power, int limbs)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int y = blockIdx.y;
    const u64 q = mods[y].q;
    const u64 part = (u64) limbs << n_power;
    const u64 loc = n + ((u64) y << n_power) + 2 * part * blockIdx.z;
    u64x2 a0 = carry ? ld2(carry + loc) : u64x2{0, 0};
    u64x2 a1 = (carry && sum_second) ? ld2(carry + loc + part) : u64x2{0, 0};
    for (int j = 0; j < k; j++) {
        const u64* p = sh.p[j];
        a0 = add2(a0, ld2(p + loc), q);
        if (fold) a0 = add2(a0, ld2(p + loc + part), q);
        if (sum_second) a1 = add2(a1, ld2(p + loc + part), q);
    }
    st2(out + loc, a0);
    if (sum_second) st2(out + loc + part, a1);
    else if (second) st2(out + loc + part, ld2(second + loc + part));
}

hipError_t kg_mpc_accumulate(u64* out, const u64* const* shares, int k, const u64* second, int fold, int sum_second,
                             const Mod* mods, int n_power, int limbs, int units, hipStream_t st)
{
    return each_share_group(shares, k, [&](const MpcShares& sh, int cnt, bool first) {
        hipLaunchKernelGGL(k_kg_mpc_accumulate, vec_grid(n_power, limbs, units), dim3(KG_THREADS), 0, st, out, sh, cnt,
                           first ? nullptr : out, first ? second : nullptr, fold, sum_second, mods, n_power, limbs);
    });
}

// A party's share, one per ciphertext of the batch, both halves in one pass (the reference: sk_multiplication and
// `addition` per half, temporaries; partial_decrypt_stage_1, ckks/mpcmanager.cu:1483-1540, also copies c0):
//   y < l:   h0[y]     = c1[y] * s[y]                      (+ what h0 holds: the transformed error)
//   y >= l:  h1[y - l] = -(a[y - l] * s[y - l])            (+ what h1 holds), a drawn from the crs: item b takes stream
//            crs_stream + b, limb j, coefficient n at index j N + n -- kg_uniform's order for one polynomial
// share [batch][l + limbs][N]; c1 of item b at c1 + b * c1_stride (may be the share's own first half, add = 0).  A
// collective decryption's share is h0 alone (limbs = 0), a refresh share carries both.  y is blockIdx.y: the branch is
// uniform per workgroup.
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_share(u64* share, const u64* c1, u64 c1_stride,
                                                             const u64* __restrict__ sk, const Mod* __restrict__ mods,
                                                             int n_power, int l, int limbs, DrbgKey crs, u64 crs_stream,
                                                             int add)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int y = blockIdx.y, b = blockIdx.z;
    const int j = y < l ? y : y - l;
    const Mod m = mods[j];
    const u64 lane = n + ((u64) j << n_power);
    u64* dst = share + (((u64) b * (l + limbs) + y) << n_power) + n;
    const u64x2 s = ld2(sk + lane);
    u64x2 v;
    if (y < l) {
        v = mul2(ld2(c1 + lane + c1_stride * b), s, m);
    } else {
        const u64 at = ((u64) j << n_power) + n;
        const u64x2 a{drbg_uniform(crs, crs_stream + b, at, m), drbg_uniform(crs, crs_stream + b, at + 1, m)};
        v = sub2(u64x2{0, 0}, mul2(a, s, m), m.q);
    }
    if (add) v = add2(v, ld2(dst), m.q);
    st2(dst, v);
}

hipError_t kg_mpc_share(u64* share, const u64* c1, u64 c1_stride, const u64* sk, const Mod* mods, int n_power, int l,
                        int limbs, int batch, DrbgKey crs, u64 crs_stream, int add, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_mpc_share, vec_grid(n_power, l + limbs, batch), dim3(KG_THREADS), 0, st, share, c1,
                       c1_stride, sk, mods, n_power, l, limbs, crs, crs_stream, add);
    return hipGetLastError();
}

// BFV shares live in the coefficient domain (bfv/mpcmanager.cu:1440-1519), where the error needs no transform: it
// is drawn here, one value per (ciphertext, coefficient), and added to every limb of h = INTT(NTT(c1) * s)
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_add_gaussian(u64* __restrict__ h, const Mod* __restrict__ mods,
                                                                    int n_power, int limbs, DrbgKey seed, u64 stream,
                                                                    GaussCdt cdt)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int b = blockIdx.y;
    const int v0 = drbg_gaussian(seed, stream, ((u64) b << n_power) + n, cdt);
    const int v1 = drbg_gaussian(seed, stream, ((u64) b << n_power) + n + 1, cdt);
    for (int j = 0; j < limbs; j++) {
        const u64 q = mods[j].q;
        u64* p = h + (((u64) b * limbs + j) << n_power) + n;
        st2(p, add2(ld2(p), u64x2{lift_small(v0, q), lift_small(v1, q)}, q));
    }
}

hipError_t kg_mpc_add_gaussian(u64* h, const Mod* mods, int n_power, int limbs, int batch, DrbgKey seed, u64 stream,
                               const GaussCdt& cdt, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_mpc_add_gaussian, vec_grid(n_power, batch, 1), dim3(KG_THREADS), 0, st, h, mods, n_power,
                       limbs, seed, stream, cdt);
    return hipGetLastError();
}

// The coordinator's k-way sums (partial_decrypt_stage_2, ckks/mpcmanager.cu:1542-1573: k `addition` launches over a
// temporary) in one launch.  Item b, limb y of share j at sh.p[j] + b * sh_stride + sh_off + y * N -- a refresh share is
// read one half at a time:
//   out[b][y] = base[b][y] + sum_j share_j[b][y]     (out items out_stride apart, base items base_stride apart)
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_sum(u64* out, u64 out_stride, const u64* base, u64 base_stride,
                                                           MpcShares sh, int k, u64 sh_stride, u64 sh_off,
                                                           const Mod* __restrict__ mods, int n_power)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int y = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[y].q;
    const u64 lane = n + ((u64) y << n_power);
    u64x2 acc = ld2(base + lane + base_stride * b);
    for (int j = 0; j < k; j++) acc = add2(acc, ld2(sh.p[j] + sh_stride * b + sh_off + lane), q);
    st2(out + lane + out_stride * b, acc);
}

hipError_t kg_mpc_sum(u64* out, u64 out_stride, const u64* base, u64 base_stride, const u64* const* shares, int k,
                      u64 sh_stride, u64 sh_off, const Mod* mods, int n_power, int limbs, int batch, hipStream_t st)
{
    return each_share_group(shares, k, [&](const MpcShares& sh, int cnt, bool first) {
        hipLaunchKernelGGL(k_kg_mpc_sum, vec_grid(n_power, limbs, batch), dim3(KG_THREADS), 0, st, out, out_stride,
                           first ? base : out, first ? base_stride : out_stride, sh, cnt, sh_stride, sh_off, mods,
                           n_power);
    });
}

// BFV: the same sum feeding the scale-and-round stage of k_kg_bfv_decryption (bfv/mpcmanager.cu:1521-1561 runs k
// `addition` launches, then decryption_fusion_bfv_kernel); item b of share j at sh.p[j] + b * sh_stride (a decryption
// share, or the h0 half of a refresh share); plain [batch][N] mod t, k <= KG_MPC_MAX_SHARES
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_bfv_round(u64* __restrict__ plain, const u64* __restrict__ c0,
                                                                 u64 c0_stride, MpcShares sh, int k, u64 sh_stride,
                                                                 const Mod* __restrict__ mods, BfvDecryptDev d,
                                                                 int n_power, int limbs)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int b = blockIdx.y;
    u64 t0 = 0, g0 = 0, t1 = 0, g1 = 0;
    for (int i = 0; i < limbs; i++) {
        const Mod m = mods[i];
        const u64 lane = n + ((u64) i << n_power);
        u64x2 acc = ld2(c0 + lane + c0_stride * b);
        for (int j = 0; j < k; j++) acc = add2(acc, ld2(sh.p[j] + sh_stride * b + lane), m.q);
        bfv_round_limb(acc.x, i, m, d, t0, g0);
        bfv_round_limb(acc.y, i, m, d, t1, g1);
    }
    st2(plain + ((u64) b << n_power) + n, u64x2{bfv_round_finish(t0, g0, d), bfv_round_finish(t1, g1, d)});
}

hipError_t kg_mpc_bfv_round(u64* plain, const u64* c0, u64 c0_stride, const u64* const* shares, int k, u64 sh_stride,
                            const Mod* mods, const BfvDecryptDev& d, int n_power, int limbs, int batch, hipStream_t st)
{
    return each_share_group(shares, k, [&](const MpcShares& sh, int cnt, bool) {
        hipLaunchKernelGGL(k_kg_mpc_bfv_round, vec_grid(n_power, batch, 1), dim3(KG_THREADS), 0, st, plain, c0, c0_stride,
                           sh, cnt, sh_stride, mods, d, n_power, limbs);
    });
}

// ---- collective refresh ("distributed bootstrapping", {ckks,bfv}/mpcmanager.cu:1575-1903 / 1563-1752; kernels
// decryption.cu:480-667).  A share is two polynomials per ciphertext: h0 over the ciphertext's limbs and h1 over all
// Q, both carrying the party's mask M with opposite signs.  The common `a` is never stored on the party's side: every
// kernel that needs it draws it from the crs in place: item b takes stream id crs_stream + b (limb j, coefficient n at
// index j N + n -- kg_uniform's order for one polynomial), and stream ids stream + 3 b .. + 3 b + 2 of the party's own
// generator (e0, e1, mask; coefficient n at index n).  A batch of B items therefore draws what B calls of one item draw.

// the `bits`-bit mask of one coefficient as the unsigned integer raw = M + 2^(bits - 1) in [0, 2^bits): the 128 bits of
// one DRBG block, cut to size
__device__ __forceinline__ void refresh_mask_raw(const DrbgKey& seed, u64 stream, u64 index, int bits, u64& hi, u64& lo)
{
    const DrbgOut o = drbg_block(seed, stream, index);
    lo = (u64) o.w[0] | ((u64) o.w[1] << 32);
    hi = (u64) o.w[2] | ((u64) o.w[3] << 32);
    if (bits < 64) {
        lo &= (1ull << bits) - 1;
        hi = 0;
    } else {
        hi &= (1ull << (bits - 64)) - 1;
    }
}

// CKKS sampler: share[b] = [ (e0 - M) mod q_j, j < l | (e1 + M) mod q_j, j < Q ], coefficient domain; e0, e1 rounded
// Gaussians (streams +0, +1 of the item), M uniform in [-2^(bits-1), 2^(bits-1)) (stream +2).  One pass, no mask buffer.
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_refresh_noise(u64* __restrict__ share,
                                                                     const Mod* __restrict__ mods, int n_power, int l,
                                                                     int limbs, DrbgKey seed, u64 stream, GaussCdt cdt,
                                                                     int bits)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int b = blockIdx.y;
    const u64 at = n;
    stream += 3 * (u64) b;
    const int e00 = drbg_gaussian(seed, stream, at, cdt), e01 = drbg_gaussian(seed, stream, at + 1, cdt);
    const int e10 = drbg_gaussian(seed, stream + 1, at, cdt), e11 = drbg_gaussian(seed, stream + 1, at + 1, cdt);
    u64 h0, l0, h1, l1;
    refresh_mask_raw(seed, stream + 2, at, bits, h0, l0);
    refresh_mask_raw(seed, stream + 2, at + 1, bits, h1, l1);
    const u64 half_hi = bits > 64 ? 1ull << (bits - 65) : 0, half_lo = bits > 64 ? 0 : 1ull << (bits - 1);
    u64* item = share + (((u64) b * (l + limbs)) << n_power) + n;
    for (int j = 0; j < limbs; j++) {
        const Mod m = mods[j];
        const u64 half = reduce128(half_hi, half_lo, m);
        const u64x2 mask{sub_mod(reduce128(h0, l0, m), half, m.q), sub_mod(reduce128(h1, l1, m), half, m.q)};
        st2(item + ((u64) (l + j) << n_power), add2(u64x2{lift_small(e10, m.q), lift_small(e11, m.q)}, mask, m.q));
        if (j < l) st2(item + ((u64) j << n_power), sub2(u64x2{lift_small(e00, m.q), lift_small(e01, m.q)}, mask, m.q));
    }
}

hipError_t kg_mpc_refresh_noise(u64* share, const Mod* mods, int n_power, int l, int limbs, int batch, DrbgKey seed,
                                u64 stream, const GaussCdt& cdt, int mask_bits, hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_mpc_refresh_noise, vec_grid(n_power, batch, 1), dim3(KG_THREADS), 0, st, share, mods,
                       n_power, l, limbs, seed, stream, cdt, mask_bits);
    return hipGetLastError();
}

// BFV shares live in the coefficient domain: after the inverse transform of both halves
//   h0[b][j] += e0 - D(M),  h1[b][j] += e1 + D(M),   M uniform in [0, t)^N (stream +2), e0 / e1 streams +0 / +1
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_refresh_bfv_noise(u64* __restrict__ share,
                                                                         const Mod* __restrict__ mods,
                                                                         const u64* __restrict__ coeff_div,
                                                                         BfvPlainScale p, Mod plain, int n_power,
                                                                         int limbs, DrbgKey seed, u64 stream,
                                                                         GaussCdt cdt)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int b = blockIdx.y;
    const u64 at = n;
    stream += 3 * (u64) b;
    const int e00 = drbg_gaussian(seed, stream, at, cdt), e01 = drbg_gaussian(seed, stream, at + 1, cdt);
    const int e10 = drbg_gaussian(seed, stream + 1, at, cdt), e11 = drbg_gaussian(seed, stream + 1, at + 1, cdt);
    const u64 m0 = drbg_uniform(seed, stream + 2, at, plain), m1 = drbg_uniform(seed, stream + 2, at + 1, plain);
    u64* item = share + (((u64) b * 2 * limbs) << n_power) + n;
    for (int j = 0; j < limbs; j++) {
        const Mod m = mods[j];
        const u64 cd = coeff_div[j];
        const u64x2 d{bfv_scaled_plain(m0, m, cd, p), bfv_scaled_plain(m1, m, cd, p)};
        u64* p0 = item + ((u64) j << n_power);
        u64* p1 = p0 + ((u64) limbs << n_power);
        st2(p0, add2(ld2(p0), sub2(u64x2{lift_small(e00, m.q), lift_small(e01, m.q)}, d, m.q), m.q));
        st2(p1, add2(ld2(p1), add2(u64x2{lift_small(e10, m.q), lift_small(e11, m.q)}, d, m.q), m.q));
    }
}

hipError_t kg_mpc_refresh_bfv_noise(u64* share, const Mod* mods, const u64* coeff_div, const BfvPlainScale& p,
                                    int n_power, int limbs, int batch, DrbgKey seed, u64 stream, const GaussCdt& cdt,
                                    hipStream_t st)
{
    hipLaunchKernelGGL(k_kg_mpc_refresh_bfv_noise, vec_grid(n_power, batch, 1), dim3(KG_THREADS), 0, st, share, mods,
                       coeff_div, p, make_mod(p.t), n_power, limbs, seed, stream, cdt);
    return hipGetLastError();
}

// Exact centred lift of t [batch][l][N] (coefficient domain, basis q_0..q_{l-1}) into out [batch][limbs][N] (items
// out_stride apart): with x the integer in (-M/2, M/2) that t stands for, M = q_0 ... q_{l-1}, limb j of the result is
// x mod q_j.  Limbs below l are copies.  For the others the coefficient is composed into words (the CKKS decoder's
// crt_compose_words: the canonical value in [0, M) and on which side of (M + 1) / 2 it lies), the words are reduced by
// Horner's rule in base 2^64, and M mod q_j -- reduced the same way -- is subtracted when x is negative.  Integer
// arithmetic throughout: the result is a function of t alone.  One thread per coefficient, one wavefront per workgroup,
// LMAX as in encode.hip.
template <int LMAX>
__global__ __launch_bounds__(EN_COMPOSE_THREADS) void k_kg_mpc_refresh_lift(u64* __restrict__ out, u64 out_stride,
                                                                            const u64* __restrict__ t,
                                                                            const Mod* __restrict__ mods,
                                                                            const u64* __restrict__ Mi_inv,
                                                                            const u64* __restrict__ Mi,
                                                                            const u64* __restrict__ upper_half,
                                                                            const u64* __restrict__ M, int l, int limbs,
                                                                            int n_power)
{
    const u64 idx = (u64) blockIdx.x * EN_COMPOSE_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    const u64* src = t + (((u64) b * l) << n_power);
    u64* dst = out + out_stride * b + idx;
    __shared__ u64 tl[LMAX * EN_COMPOSE_THREADS];
    u64 acc[LMAX];
    const bool negative = crt_compose_words<LMAX>(acc, src, idx, mods, Mi_inv, Mi, upper_half, M, l, n_power, tl);
    for (int j = 0; j < l; j++) dst[(u64) j << n_power] = src[idx + ((u64) j << n_power)];
    // the words go back to the thread's own column of `tl` (free once the value is composed): the loops below index them
    // by a run-time k, which registers cannot be
#pragma unroll
    for (int k = 0; k < LMAX; k++) {
        if (k < l) tl[k * EN_COMPOSE_THREADS + threadIdx.x] = acc[k];
    }
    for (int j = l; j < limbs; j++) {
        const Mod m = mods[j];
        u64 r = 0, mr = 0;
        for (int k = l - 1; k >= 0; k--) {
            r = reduce128(r, tl[k * EN_COMPOSE_THREADS + threadIdx.x], m);
            mr = reduce128(mr, M[k], m);
        }
        dst[(u64) j << n_power] = negative ? sub_mod(r, mr, m.q) : r;
    }
}

hipError_t kg_mpc_refresh_lift(u64* out, u64 out_stride, const u64* t, const Mod* mods, const u64* Mi_inv,
                               const u64* Mi, const u64* upper_half, const u64* M, int l, int limbs, int n_power,
                               int batch, hipStream_t st)
{
    if (l > EN_MAX_WORDS) return hipErrorInvalidValue;
    const dim3 grid((1u << n_power) / EN_COMPOSE_THREADS, batch), block(EN_COMPOSE_THREADS);
#define KG_LIFT(LM) hipLaunchKernelGGL(k_kg_mpc_refresh_lift<LM>, grid, block, 0, st, out, out_stride, t, mods, Mi_inv, Mi, upper_half, M, l, limbs, n_power)
    if (l <= 8) KG_LIFT(8);
    else if (l <= 16) KG_LIFT(16);
    else if (l <= 32) KG_LIFT(32);
    else KG_LIFT(EN_MAX_WORDS);
#undef KG_LIFT
    return hipGetLastError();
}

// The refreshed ciphertext, out [batch][2][limbs][N] (items out_stride apart):
//   part 0 = (add_out: what it holds -- the lifted polynomial, or an earlier group's sum) + sum_j h1_j
//            (+ D(plain[b]), BFV: plain [batch][N] mod t);   part 1 = a, drawn from the crs as the parties drew it
//            (write_a; NTT domain)
__global__ __launch_bounds__(KG_THREADS) void k_kg_mpc_refresh_finish(u64* out, u64 out_stride, MpcShares sh, int k,
                                                                      u64 sh_stride, u64 sh_off, int add_out,
                                                                      const u64* __restrict__ plain,
                                                                      const u64* __restrict__ coeff_div,
                                                                      BfvPlainScale p, const Mod* __restrict__ mods,
                                                                      int n_power, DrbgKey crs, u64 crs_stream,
                                                                      int write_a)
{
    const u64 n = ((u64) blockIdx.x * KG_THREADS + threadIdx.x) * KG_VEC;
    const int y = blockIdx.y, b = blockIdx.z, limbs = gridDim.y;
    const Mod m = mods[y];
    const u64 lane = n + ((u64) y << n_power);
    u64* dst = out + out_stride * b + lane;
    u64x2 acc = add_out ? ld2(dst) : u64x2{0, 0};
    for (int j = 0; j < k; j++) acc = add2(acc, ld2(sh.p[j] + sh_stride * b + sh_off + lane), m.q);
    if (plain) {
        const u64x2 v = ld2(plain + ((u64) b << n_power) + n);
        const u64 cd = coeff_div[y];
        acc = add2(acc, u64x2{bfv_scaled_plain(v.x, m, cd, p), bfv_scaled_plain(v.y, m, cd, p)}, m.q);
    }
    st2(dst, acc);
    if (write_a) {
        const u64 at = ((u64) y << n_power) + n;
        st2(dst + ((u64) limbs << n_power),
            u64x2{drbg_uniform(crs, crs_stream + b, at, m), drbg_uniform(crs, crs_stream + b, at + 1, m)});
    }
}

hipError_t kg_mpc_refresh_finish(u64* out, u64 out_stride, const u64* const* shares, int k, u64 sh_stride, u64 sh_off,
                                 int add_out, const u64* plain, const u64* coeff_div, const BfvPlainScale& p,
                                 const Mod* mods, int n_power, int limbs, int batch, DrbgKey crs, u64 crs_stream,
                                 hipStream_t st)
{
    return each_share_group(shares, k, [&](const MpcShares& sh, int cnt, bool first) {
        hipLaunchKernelGGL(k_kg_mpc_refresh_finish, vec_grid(n_power, limbs, batch), dim3(KG_THREADS), 0, st, out,
                           out_stride, sh, cnt, sh_stride, sh_off, first ? add_out : 1, first ? plain : nullptr,
                           coeff_div, p, mods, n_power, crs, crs_stream, first ? 1 : 0);
    });
}

} // namespace hegpu
