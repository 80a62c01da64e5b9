// ckks_const.cuh -- a double in the kernel arguments -> the residue of its nearest integer, for the kernels that add or
// multiply a constant into every slot of an NTT-domain CKKS ciphertext (keygen.hip k_kg_ckks_constant / k_kg_ckks_gaussian,
// rns.hip k_ckks_weighted_sum / k_ckks_double_sub / k_gate_combine).  One definition, so that all of them give the same residues.
#pragma once
#include "modarith.cuh"

namespace hegpu {

// c mod q for a non-negative integer-valued double c < 2^128, from its two 64-bit halves
__device__ __forceinline__ u64 magnitude_residue(double c, const Mod& m)
{
    const double two64 = 18446744073709551616.0;
    const u64 lo = (u64) fmod(c, two64), hi = (u64) (c / two64);
    return reduce128(hi, lo, m);
}

// round(value) mod q for |value| < 2^128, the constant of addition_constant_plain_ckks_poly and its kin (addition.cu:219-300,
// multiplication.cu:333-372).  A negative value with residue 0 gives q, not 0: sub(q, 0) == q is the reference's (SURVEY 8c
// quirk 1); add_mod / sub_mod / mul_barrett take it.
__device__ __forceinline__ u64 real_constant_residue(double value, const Mod& m)
{
    const double c = round(value);
    const u64 pt = magnitude_residue(fabs(c), m);
    return signbit(c) ? sub_mod(m.q, pt, m.q) : pt;
}

// The reference turns the rounded doubles of a Gaussian integer into residues with NTL big integers (ckks/operator.cu:583-617)
// and accepts any magnitude; a double is mant * 2^e: below 2^128 the residue is magnitude_residue, beyond that
// (mant mod q) * (2^e mod q) -- exact for every finite double.  A negative value gives the non-negative residue (0 for -0).
__device__ __forceinline__ u64 residue_of_rounded(double value, const Mod& m)
{
    double c = round(value);
    const bool neg = signbit(c);
    c = fabs(c);
    const double two64 = 18446744073709551616.0;
    u64 r;
    if (c < two64 * two64) {
        r = magnitude_residue(c, m);
    } else {
        int e;
        const double fr = frexp(c, &e);              // c = fr * 2^e, 0.5 <= fr < 1
        const u64 mant = (u64) ldexp(fr, 53);        // the 53-bit integer mantissa, exact
        r = reduce64(mant, m);
        u64 p = reduce64(2, m), acc = reduce64(1, m); // 2^(e - 53) mod q by square and multiply
        for (int sh = e - 53; sh; sh >>= 1) {
            if (sh & 1) acc = reduce128(mulhi64(acc, p), acc * p, m);
            p = reduce128(mulhi64(p, p), p * p, m);
        }
        r = reduce128(mulhi64(r, acc), r * acc, m);
    }
    return (neg && r) ? m.q - r : r; // NTL: (x % q) made non-negative
}

// The slot constant round(re) + round(im) i: in the NTT domain i is +psi^(N/2) on the first half of the positions and
// -psi^(N/2) on the second (cipher_add_by_gaussian_integer_kernel / cipher_mult_by_gaussian_integer_kernel,
// multiplication.cu:497-570)
__device__ __forceinline__ u64 gaussian_slot_constant(double re, double im, u64 psi_half, bool first_half, const Mod& m)
{
    const u64 c_real = residue_of_rounded(re, m), c_imag = residue_of_rounded(im, m);
    const u64 const_imag = mul_barrett(c_imag, psi_half, m);
    return first_half ? add_mod(c_real, const_imag, m.q) : sub_mod(c_real, const_imag, m.q);
}

} // namespace hegpu
