// bfv_plain.cuh -- the scaled BFV plaintext D(m) = floor(Q / t) * m + the rounding fix, for every kernel that adds a
// plaintext (or the constant one) to a coefficient-domain ciphertext (keygen.hip k_kg_bfv_message_add /
// k_kg_bfv_plain_addsub / the collective refresh, rns.hip k_gate_combine).  One definition, so that all of them give the
// same residues.
#pragma once
#include "modarith.cuh"

namespace hegpu {

// the scalars of the scaled plaintext D(m) = Delta * m + the rounding fix (ops.cpp: bfv_plain_scale)
struct BfvPlainScale {
    u64 Q_mod_t, upper_threshold, t;
};

// D(m): limb y of the scaled plaintext, Delta * m + the rounding fix (tail of enc_div_lastq_bfv_kernel,
// encryption.cu:158-172).  The 64-bit wrap-around and the detour through `int` are the reference's (:160-163).
__device__ __forceinline__ u64 bfv_scaled_plain(u64 message, const Mod& m, u64 coeff_div, const BfvPlainScale& p)
{
    u64 fix = message * p.Q_mod_t;
    fix = fix + p.upper_threshold;
    fix = (u64) (long long) (int) (fix / p.t);
    return add_mod(mul_barrett(message, coeff_div, m), fix, m.q);
}

} // namespace hegpu
