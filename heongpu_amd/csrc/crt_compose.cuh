// crt_compose.cuh -- multi-word CRT composition of one RNS coefficient (device), shared by the CKKS decoder
// (encode.hip) and the exact centred lift of the collective refresh (keygen.hip).
#pragma once
#include "modarith.cuh"

namespace hegpu {

// ---- CRT composition (encode_kernel_compose, encoding.cu:234-383; biginteger helpers
// util/bigintegerarith.cuh): little-endian 64-bit words, at most EN_MAX_WORDS of them
#define EN_MAX_WORDS 64

// one wavefront per workgroup: a thread is one long dependent chain -- l mul_barrett + l x l multiply-accumulate words --
// so the launch is spread over as many CUs as it has wavefronts (N = 2^14: 256 workgroups, one per CU)
#define EN_COMPOSE_THREADS 64
// LMAX: compile-time bound on the word count l, so that the accumulator lives in registers (every index below is static:
// the word loops are fully unrolled with `k < l` guards).  Rounds 1-5 kept acc[64] in scratch memory and ran two values
// per thread: 86 us at N = 2^14 -- more than the rest of a decode together.  The integers are the same whatever the
// order of evaluation (each partial sum is brought below M, its canonical value), and the final conversion adds the words
// in the reference's order.
// crt_compose_words: acc[0..l) = the value of coefficient `at` of plain [l][N] in [0, M), little-endian words;
// returns whether it lies in the upper half (acc >= upper_half = (M + 1) >> 1), i.e. stands for acc - M
template <int LMAX>
__device__ __forceinline__ bool crt_compose_words(u64 (&acc)[LMAX], const u64* __restrict__ plain, u64 at,
                                                  const Mod* __restrict__ mods, const u64* __restrict__ Mi_inv,
                                                  const u64* __restrict__ Mi, const u64* __restrict__ upper_half,
                                                  const u64* __restrict__ M, int l, int n_power, u64* tl)
{
    // The l residues of the value are requested TOGETHER (unrolled, independent loads) and their products with Mi_inv parked
    // in the thread's own column of `tl` -- inside the word loop below each would cost a full memory latency per limb
    // (measured: 26 us of a 28 us kernel at N = 2^14).  A thread reads back only what it wrote itself: no barrier.
#pragma unroll
    for (int k = 0; k < LMAX; k++) {
        if (k < l) tl[k * EN_COMPOSE_THREADS + threadIdx.x] = mul_barrett(plain[at + ((u64) k << n_power)], Mi_inv[k], mods[k]);
    }
    // Round 6: the l terms are summed WITHOUT a comparison / subtraction after each (the reference brings every partial sum
    // below M: l compares + up to l subtractions of l words each, 40 % of the instructions at l = 9).  The sum is below
    // l M < 2^(64 l + 6): one more word (`top`).  Its quotient by M is floor(sum_i t_i / q_i) -- sum_i t_i M / q_i over M -- which
    // a double-precision sum of the l fractions gives to within one (absolute error below l 2^-51: wrong only when the true
    // sum sits that close to an integer, and then by exactly one); ONE multiply-subtract of ke M and one correction (add M
    // back if the difference went negative, subtract M once more if it is still >= M) leave the canonical value in [0, M) --
    // the same integer the reference's chain of reductions ends with.
    u64 top = 0;
#pragma unroll
    for (int k = 0; k < LMAX; k++) acc[k] = 0;
    double tf = 0.0;
    for (int i = 0; i < l; i++) {
        const u64 t = tl[i * EN_COMPOSE_THREADS + threadIdx.x];
        tf += (double) t * (1.0 / (double) mods[i].q);
        const u64* mi = Mi + (u64) i * l;
        u64 carry = 0;
#pragma unroll
        for (int k = 0; k < LMAX; k++) {
            if (k < l) {
                u64 hi, lo;
                mul64wide(mi[k], t, hi, lo);
                const u64 s1 = lo + carry;
                const u64 c1 = s1 < lo;
                const u64 s2 = acc[k] + s1;
                const u64 c2 = s2 < s1;
                acc[k] = s2;
                carry = hi + c1 + c2;
            }
        }
        top += carry;
    }
    {
        const u64 ke = (u64) tf; // <= l
        u64 borrow = 0, mcarry = 0;
#pragma unroll
        for (int k = 0; k < LMAX; k++) {
            if (k < l) {
                u64 hi, lo;
                mul64wide(M[k], ke, hi, lo);
                const u64 sub = lo + mcarry; // word k of ke M
                mcarry = hi + (sub < lo);
                const u64 d = acc[k] - sub;
                const u64 b1 = acc[k] < sub;
                const u64 d2 = d - borrow;
                const u64 b2 = d < borrow;
                acc[k] = d2;
                borrow = b1 | b2;
            }
        }
        top = top - mcarry - borrow; // 0, or all ones when ke was one too large
        bool geq = true, decided = false; // acc >= M ?  (most significant differing word decides)
#pragma unroll
        for (int k = LMAX - 1; k >= 0; k--) {
            if (k < l && !decided && acc[k] != M[k]) {
                geq = acc[k] > M[k];
                decided = true;
            }
        }
        const bool negative = top != 0;
        if (negative || geq) { // acc += M  or  acc -= M
            u64 c = 0;
#pragma unroll
            for (int k = 0; k < LMAX; k++) {
                if (k < l) {
                    const u64 m = M[k];
                    if (negative) {
                        const u64 s1 = acc[k] + m;
                        const u64 c1 = s1 < m;
                        const u64 s2 = s1 + c;
                        const u64 c2 = s2 < s1;
                        acc[k] = s2;
                        c = c1 | c2;
                    } else {
                        const u64 d = acc[k] - m;
                        const u64 b1 = acc[k] < m;
                        const u64 d2 = d - c;
                        const u64 b2 = d < c;
                        acc[k] = d2;
                        c = b1 | b2;
                    }
                }
            }
        }
    }
    bool upper = true, decided = false;
#pragma unroll
    for (int k = LMAX - 1; k >= 0; k--) {
        if (k < l && !decided && acc[k] != upper_half[k]) {
            upper = acc[k] > upper_half[k];
            decided = true;
        }
    }
    return upper;
}

} // namespace hegpu
