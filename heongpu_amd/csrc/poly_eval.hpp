// poly_eval.hpp -- host only: the evaluation order of a polynomial on a CKKS ciphertext.  No device,
// no context: integers and FP64 on the host.
//
// The schedule is the reference's (HEOperator<CKKS>::evaluate_poly, gen_power, evaluate_poly_recurse,
// evaluate_poly_from_polynomial_basis and Polynomial::split_coeffs, ckks/operator.cu:4292-4671, :6633-6678): baby powers
// 2^s - 1 .. 1 and giant powers 2^s .. 2^(D-1) with s = optimal_split(D), then the recursive split q * x^(2^j) + r down to
// leaves of degree < 2^s.  A level is the index of a ciphertext's last prime (limbs = level + 1), a scale the factor its
// slots carry.  The plan is a flat list of steps over numbered registers; register 0 is the input (power 1), every step
// writes a new register, the last step's register is the result.
//
// Two departures, both where the reference reads a power it never made:
//   * D = bit length of the degree (ceil(log2(degree + 1))).  The reference takes ceil(log2(degree)), which is the same
//     number unless the degree is a power of two; there its first split needs x^degree and only x^(degree/2) exists.
//   * the threshold of the conditional rescale of q (:4545) is target_scale / 2; the reference compares with the scale
//     of its bootstrapping context, which is the scale it calls the evaluator with.
#pragma once
#include "../../include/hegpu.h"
#include <complex>
#include <cstdint>
#include <vector>

namespace hegpu {
namespace host {

enum { POLY_MONOMIAL = 0, POLY_CHEBYSHEV = 1 };
enum { POLY_STEP_POWER = 0, POLY_STEP_LEAF = 1, POLY_STEP_COMBINE = 2 };
enum { POLY_TAIL_NONE = -1, POLY_TAIL_ONE = -2 }; // PolyStep::c of a POWER step that subtracts no register
constexpr int POLY_LEAF_MAX = 15;                 // power terms of one leaf: 15 products and w_0 fit the 128-bit sum

// One step of a plan is the C ABI's struct (include/hegpu.h states every field); kind is a POLY_STEP_*.
using PolyStep = ::hegpu_poly_step;
static_assert(sizeof(PolyStep::term_reg) / sizeof(int32_t) == POLY_LEAF_MAX && sizeof(PolyStep::w) / sizeof(double[2]) == POLY_LEAF_MAX,
              "a leaf of hegpu_poly_step holds POLY_LEAF_MAX terms");

// std::invalid_argument: degree < 2, basis not one of the two, max_deg < degree, a non-finite coefficient or scale, a
// scale <= 0, a leaf of more than POLY_LEAF_MAX power terms, fewer levels than the schedule spends (a level below 0, or
// a rescale at level 0), level >= the number of primes.
std::vector<PolyStep> poly_eval_plan(int basis, const std::vector<std::complex<double>>& coeffs, int max_deg, bool lead,
                                     int level, double scale, double target_scale, const std::vector<uint64_t>& primes);

// EvalMod of CKKS bootstrapping (eval_mod, ckks/operator.cu:4248-4290) as a plan the same executor runs.  The input
// register holds u in [-1, 1] with K u = I + eps, I an integer below K in magnitude.  With c = (1 / 2 pi)^(1 / 2^r) the plan
// evaluates p, the degree-`degree` Chebyshev interpolant (at the Chebyshev nodes, in doubles) of
//     g(u) = c cos(2 pi (K u - 1/4) / 2^r),
// and then r double-angle steps y <- 2 y^2 - c^(2^(i+1)), each a POWER step with a = b = the previous register,
// POLY_TAIL_ONE and tail_const = c^(2^(i+1)) at the step's scale: y_r = sin(2 pi eps) / 2 pi.  p gets the target scale of
// the reference's square-root chain (:4257-4265), so that the result carries target_scale (to the rounding of doubles).
// The reference's change of variable by a constant addition (:4267-4271) is inside g.
// std::invalid_argument: K < 1, double_angle outside [0, 8], a degree poly_eval_plan refuses, fewer levels than
// bit_length(degree) + double_angle, a non-finite or non-positive scale.
std::vector<PolyStep> eval_mod_plan(int K, int degree, int double_angle, int level, double scale, double target_scale,
                                    const std::vector<uint64_t>& primes);

// The same plan for alpha + A cos(2 pi (K u - phase)): the interpolant of g(u) = c cos(2 pi (K u - phase) /
// 2^r) with c = A^(1 / 2^r), then the r double-angle steps; the last tail constant is A - alpha in place of A (any sign, or
// zero), and without a double angle alpha is added to Chebyshev coefficient 0.  eval_mod_plan is (1/4, 1 / 2 pi, 0), step for
// step.  std::invalid_argument: what eval_mod_plan refuses, an amplitude <= 0, a non-finite phase, amplitude or offset.
std::vector<PolyStep> eval_trig_plan(int K, int degree, int double_angle, double phase, double amplitude, double offset,
                                     int level, double scale, double target_scale, const std::vector<uint64_t>& primes);

} // namespace host
} // namespace hegpu
