/*
 * gpuntt/common/modular_arith.cuh -- stand-in for the one GPU-NTT header that the reference's
 * switchkey.cu, multiplication.cu and addition.cu include.  TEST INFRASTRUCTURE ONLY
 * (oracle/ref_build.py compiles those three files unchanged against it).
 *
 * OWN CODE, written from the call sites in the three kernel files and from oracle/o_arith.c: GPU-NTT is
 * an empty submodule of the reference tree, so the arithmetic below is the SAME RESTATEMENT as the
 * oracle's (o_mod / o_add / o_sub / o_mult / o_reduce_forced) and is not pinned by anything here.  What
 * this header makes possible is running the reference's own kernel text -- index arithmetic, loops,
 * operand order, table use -- on top of it.
 *
 * Shape dictated by the call sites:
 *   switchkey.cu:1062      `Modulus modulus = B_prime[block_y];`   -> Modulus is a class template,
 *                                                                     Modulus64 an alias of Modulus<Data64>
 *   multiplication.cu:352  `Data64 coeff[2] = {low, high}; reduce(coeff, q)` -> reduce(const Data64*, ...)
 *                                                                     takes the 128-bit value {low, high}
 *   switchkey.cu:1130,1146 `reduce(Data64, q)` (base_conversion_BtoD_relin_kernel only; no test reaches it)
 */
#ifndef HEGPU_REF_SHIM_MODULAR_ARITH_CUH
#define HEGPU_REF_SHIM_MODULAR_ARITH_CUH

#include <cstdint>
#include <hip/hip_runtime.h>

typedef std::uint32_t Data32;
typedef std::uint64_t Data64;

/* {value, bit, mu}: bit = floor(log2 q) + 1, mu = floor(2^(2 bit + 1) / q)  (o_mod) */
template <typename T> struct Modulus
{
    T value;
    T bit;
    T mu;

    __host__ __device__ Modulus() : value(0), bit(0), mu(0) {}
    __host__ explicit Modulus(T q) : value(q), bit(0), mu(0)
    {
        while (bit < 8 * sizeof(T) && (q >> bit) != 0) bit++;
        mu = (T) ((((unsigned __int128) 1) << (2 * bit + 1)) / q);
    }
};
typedef Modulus<Data64> Modulus64;

struct OPERATOR_GPU_64
{
    /* one conditional subtraction (o_add) */
    static __host__ __device__ __forceinline__ Data64 add(Data64 a, Data64 b, const Modulus64& m)
    {
        Data64 s = a + b;
        return (s >= m.value) ? (s - m.value) : s;
    }

    /* a + q - b, one conditional subtraction: sub(q, 0) == q stays non-canonical (o_sub) */
    static __host__ __device__ __forceinline__ Data64 sub(Data64 a, Data64 b, const Modulus64& m)
    {
        Data64 d = a + m.value;
        d = d - b;
        return (d >= m.value) ? (d - m.value) : d;
    }

    /* Barrett, the sequence of o_mult: exact and canonical whenever a * b < 2^(2 bit) */
    static __host__ __device__ __forceinline__ Data64 mult(Data64 a, Data64 b, const Modulus64& m)
    {
        unsigned __int128 z = (unsigned __int128) a * b;
        unsigned __int128 w = z >> (m.bit - 2);
        w = (unsigned __int128) ((Data64) w) * m.mu;
        w = w >> (m.bit + 3);
        w = (unsigned __int128) ((Data64) w) * m.value;
        z = z - w;
        Data64 r = (Data64) z;
        return (r >= m.value) ? (r - m.value) : r;
    }

    /* full reduction of any 64-bit value (o_reduce_forced) */
    static __host__ __device__ __forceinline__ Data64 reduce_forced(Data64 a, const Modulus64& m)
    {
        return a % m.value;
    }

    /* the 128-bit value {a[0] = low word, a[1] = high word} mod q, exact for every input: the high word is
     * reduced, then the low word is shifted in bit by bit (q < 2^62, so 2 r + 1 never wraps) */
    static __host__ __device__ __forceinline__ Data64 reduce(const Data64* a, const Modulus64& m)
    {
        Data64 r = a[1] % m.value;
        Data64 lo = a[0];
        for (int i = 63; i >= 0; i--)
        {
            r = (r << 1) | ((lo >> i) & 1);
            if (r >= m.value) r -= m.value;
        }
        return r;
    }

    /* one Barrett step on a single word (the sequence of mult with the product replaced by a); only
     * base_conversion_BtoD_relin_kernel calls it, which no test here runs */
    static __host__ __device__ __forceinline__ Data64 reduce(Data64 a, const Modulus64& m)
    {
        return mult(a, 1, m);
    }
};

#endif
