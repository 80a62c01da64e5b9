// bootstrap_plan.hpp -- host only: every scale label of the CKKS refresh (reference
// generate_bootstrapping_params_v2 / regular_bootstrapping_v2, ckks/operator.cu:6906-7000, :7147-7224).  No device, no
// context: integers and FP64 on the host.  A level is the index of a ciphertext's last prime, a scale the exact label a
// ciphertext carries (as in poly_eval.hpp); the plan states what the sequence op_ckks_bootstrap does at which level and
// which scale the diagonals of every linear factor are encoded at.
//
//   input  [2][1][N] at q_0, scale D, coefficients a               integer D a + e
//   x k1   k1 = max(1, round(q_0 / (ratio D))), D' = k1 D           D' a + e',  eps = D' a / q_0
//   raise  to cts_level, labelled q_0 K                             u = (I + eps) / K in [-1, 1]
//   CoeffToSlot, factor f encoded at cts_scale[f]                   label cts_label[f] after its rescale; the last is the
//          = (S / (q_0 K))^(1/P) q_(cts_level - f), S = q_(eval_level)    sine scale S to the rounding of doubles
//   split  drops one limb, label unchanged                          level eval_level
//   EvalMod plan (eval_level, eval_in_scale, eval_target_scale = S) sin(2 pi eps) / 2 pi at eval_out_scale, stc_level
//   relabel eval_out_scale D' / q_0 = stc_in_scale                  the value is (rho / 2 pi) sin(2 pi a / rho), rho = q_0 / D'
//   merge  drops one limb; SlotToCoeff, factor g encoded at stc_scale[g]  label D at out_level
//          = (D / stc_in_scale)^(1/P) q_(stc_level - 1 - g)
#pragma once
#include "../../include/hegpu.h"
#include <cstdint>
#include <vector>

namespace hegpu {
namespace host {

constexpr int BOOTSTRAP_MAX_PIECES = 5; // the factorisation of the special FFT has 2 .. 5 pieces (encoding_transform.hpp)

// The configs and plans are the C ABI's structs (include/hegpu.h states every field).
using BootstrapConfig = ::hegpu_bootstrap_config;
using BootstrapPlan = ::hegpu_bootstrap_plan;
using SlimBootstrapConfig = ::hegpu_slim_bootstrap_config;
using SlimBootstrapPlan = ::hegpu_slim_bootstrap_plan;
static_assert(sizeof(BootstrapPlan::cts_scale) == BOOTSTRAP_MAX_PIECES * sizeof(double) &&
                  sizeof(BootstrapPlan::stc_label) == BOOTSTRAP_MAX_PIECES * sizeof(double) &&
                  sizeof(SlimBootstrapPlan::stc_scale) == BOOTSTRAP_MAX_PIECES * sizeof(double) &&
                  sizeof(SlimBootstrapPlan::cts_label) == BOOTSTRAP_MAX_PIECES * sizeof(double),
              "the plans of hegpu.h hold BOOTSTRAP_MAX_PIECES factors per transform");

// std::invalid_argument: fewer levels than P_cts + 1 + bit_length(degree) + r + 1 + P_stc and one limb left, start levels
// that do not follow from one another, K < 1, ratio D > q_0, a scale or ratio that is not positive and finite, a piece
// count outside [2, 5], what eval_mod_plan refuses.
BootstrapPlan bootstrap_plan(const BootstrapConfig& cfg, const std::vector<uint64_t>& primes);

// ---- the slim family (reference slim_bootstrapping, bit_bootstrapping, gate_bootstrapping): SlotToCoeff
// first, one EvalMod-like plan on the real parts.
//
//   input  [2][P_stc + 1][N], slots z at scale D, level in_level = P_stc
//   SlotToCoeff, factor g encoded at stc_scale[g]                   label stc_label[g] after its rescale; the last is
//          = (q_0 / (ratio D))^(1/P) q_(P_stc - g)                   q_0 / ratio to the rounding of doubles, at level 0
//   raise  to cts_level, labelled q_0 K                             t = (q_0 / ratio) a + q_0 I + e,  u = t / (q_0 K)
//   CoeffToSlot as above, then conj, then x + conj x dropping a limb    slot j holds u_j (real), level eval_level
//   trig plan (K, degree, r, phase, amplitude, offset)              offset + amplitude cos(2 pi (a / ratio - phase))
//   out    at out_level = eval_level - bit_length(degree) - r, labelled eval_out_scale (/ ratio if `arithmetic`)
// std::invalid_argument: fewer levels than P_cts + 1 + bit_length(degree) + r and one limb left, a chain of fewer than
// P_stc + 1 limbs, ratio < 2, a piece count outside [2, 5], a factor scale below 1, a scale that is not positive and
// finite, what eval_trig_plan refuses.
SlimBootstrapPlan slim_bootstrap_plan(const SlimBootstrapConfig& cfg, const std::vector<uint64_t>& primes);

} // namespace host
} // namespace hegpu
