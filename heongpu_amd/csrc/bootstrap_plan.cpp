// bootstrap_plan.cpp -- see bootstrap_plan.hpp.
#include "bootstrap_plan.hpp"

#include "poly_eval.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace hegpu {
namespace host {

namespace {
int bootstrap_bit_length(int v)
{
    int b = 0;
    while (v > 0) { b++; v >>= 1; }
    return b;
}
bool bootstrap_scale_ok(double v) { return std::isfinite(v) && v > 0; }
} // namespace

BootstrapPlan bootstrap_plan(const BootstrapConfig& cfg, const std::vector<uint64_t>& primes)
{
    const int Q = (int) primes.size();
    if (Q < 1) throw std::invalid_argument("bootstrap_plan: no primes");
    for (uint64_t p : primes)
        if (p < 2) throw std::invalid_argument("bootstrap_plan: a prime below 2");
    if (!bootstrap_scale_ok(cfg.scale) || !bootstrap_scale_ok(cfg.message_ratio))
        throw std::invalid_argument("bootstrap_plan: the scale and the message ratio are positive finite numbers");
    if (cfg.K < 1 || cfg.K > (1 << 20)) throw std::invalid_argument("bootstrap_plan: K is at least 1");
    if (cfg.sine_degree < 2 || cfg.sine_degree > 255) throw std::invalid_argument("bootstrap_plan: the sine degree is 2 .. 255");
    if (cfg.double_angle < 0 || cfg.double_angle > 8) throw std::invalid_argument("bootstrap_plan: double_angle is 0 .. 8");
    for (int p : {cfg.cts_pieces, cfg.stc_pieces})
        if (p < 2 || p > BOOTSTRAP_MAX_PIECES) throw std::invalid_argument("bootstrap_plan: the piece counts lie in [2, 5]");
    const double q0 = static_cast<double>(primes[0]);
    if (!(cfg.message_ratio * cfg.scale <= q0))
        throw std::invalid_argument("bootstrap_plan: message_ratio * scale is at most q_0");

    BootstrapPlan pl{};
    pl.K = cfg.K;
    pl.sine_degree = cfg.sine_degree;
    pl.double_angle = cfg.double_angle;
    pl.cts_pieces = cfg.cts_pieces;
    pl.stc_pieces = cfg.stc_pieces;
    pl.cts_level = cfg.cts_level;
    if (pl.cts_level < 0 || pl.cts_level >= Q) throw std::invalid_argument("bootstrap_plan: no such CoeffToSlot level");
    // the levels follow from one another: P factors and the limb the split drops; the polynomial and the double angles;
    // the limb the merge drops and P factors
    const int spent_eval = bootstrap_bit_length(cfg.sine_degree) + cfg.double_angle;
    pl.eval_level = pl.cts_level - pl.cts_pieces - 1;
    pl.stc_level = pl.eval_level - spent_eval;
    pl.out_level = pl.stc_level - 1 - pl.stc_pieces;
    if (pl.out_level < 0)
        throw std::invalid_argument("bootstrap_plan: too few levels (CoeffToSlot pieces + 1 + bit length of the sine degree + "
                                    "double angles + 1 + SlotToCoeff pieces, and one limb left)");
    if ((cfg.eval_level >= 0 && cfg.eval_level != pl.eval_level) || (cfg.stc_level >= 0 && cfg.stc_level != pl.stc_level))
        throw std::invalid_argument("bootstrap_plan: EvalMod starts pieces + 1 levels below CoeffToSlot, SlotToCoeff where "
                                    "EvalMod ends");

    // 1. the pre-multiplier
    const double k1 = std::max(1.0, std::round(q0 / (cfg.message_ratio * cfg.scale)));
    if (!(k1 < 9007199254740992.0)) throw std::invalid_argument("bootstrap_plan: the pre-multiplier left the range of a double");
    pl.k1 = static_cast<uint64_t>(k1);
    const double scale1 = k1 * cfg.scale; // D'
    // 2. the raise
    pl.raise_scale = q0 * static_cast<double>(cfg.K);
    // 3. CoeffToSlot brings the label to the sine scale
    const double S = static_cast<double>(primes[(size_t) pl.eval_level]);
    const double share = std::pow(S / pl.raise_scale, 1.0 / pl.cts_pieces);
    double label = pl.raise_scale;
    for (int f = 0; f < pl.cts_pieces; f++) {
        const double q = static_cast<double>(primes[(size_t) (pl.cts_level - f)]);
        pl.cts_scale[f] = share * q;
        label = label * pl.cts_scale[f] / q; // the product's label, then the rescale: as the sequence's caller labels it
        pl.cts_label[f] = label;
    }
    // 4. EvalMod from the label as it comes out
    pl.eval_in_scale = label;
    pl.eval_target_scale = S;
    const std::vector<PolyStep> steps = eval_mod_plan(cfg.K, cfg.sine_degree, cfg.double_angle, pl.eval_level, pl.eval_in_scale,
                                                      pl.eval_target_scale, primes);
    if (steps.back().level != pl.stc_level) throw std::invalid_argument("bootstrap_plan: EvalMod does not end at its level");
    pl.eval_out_scale = steps.back().scale;
    // 5. the value sin(2 pi eps) / 2 pi becomes (q_0 / D') times itself by its label alone
    pl.stc_in_scale = pl.eval_out_scale * scale1 / q0;
    const double back = std::pow(cfg.scale / pl.stc_in_scale, 1.0 / pl.stc_pieces);
    label = pl.stc_in_scale;
    for (int g = 0; g < pl.stc_pieces; g++) {
        const double q = static_cast<double>(primes[(size_t) (pl.stc_level - 1 - g)]);
        pl.stc_scale[g] = back * q;
        label = label * pl.stc_scale[g] / q;
        pl.stc_label[g] = label;
    }
    pl.out_scale = label;
    for (int i = 0; i < BOOTSTRAP_MAX_PIECES; i++) {
        if (i < pl.cts_pieces && !(bootstrap_scale_ok(pl.cts_scale[i]) && pl.cts_scale[i] >= 1.0))
            throw std::invalid_argument("bootstrap_plan: a CoeffToSlot factor's scale is below one or not finite");
        if (i < pl.stc_pieces && !(bootstrap_scale_ok(pl.stc_scale[i]) && pl.stc_scale[i] >= 1.0))
            throw std::invalid_argument("bootstrap_plan: a SlotToCoeff factor's scale is below one or not finite");
    }
    if (!bootstrap_scale_ok(pl.out_scale) || !bootstrap_scale_ok(pl.stc_in_scale)) throw std::invalid_argument("bootstrap_plan: a scale left the range of a double");
    return pl;
}

SlimBootstrapPlan slim_bootstrap_plan(const SlimBootstrapConfig& cfg, const std::vector<uint64_t>& primes)
{
    const int Q = (int) primes.size();
    if (Q < 1) throw std::invalid_argument("slim_bootstrap_plan: no primes");
    for (uint64_t p : primes)
        if (p < 2) throw std::invalid_argument("slim_bootstrap_plan: a prime below 2");
    if (!bootstrap_scale_ok(cfg.scale)) throw std::invalid_argument("slim_bootstrap_plan: the scale is a positive finite number");
    if (!std::isfinite(cfg.ratio) || !(cfg.ratio >= 2.0)) throw std::invalid_argument("slim_bootstrap_plan: the ratio is at least 2");
    if (cfg.K < 1 || cfg.K > (1 << 20)) throw std::invalid_argument("slim_bootstrap_plan: K is at least 1");
    if (cfg.degree < 2 || cfg.degree > 255) throw std::invalid_argument("slim_bootstrap_plan: the degree is 2 .. 255");
    if (cfg.double_angle < 0 || cfg.double_angle > 8) throw std::invalid_argument("slim_bootstrap_plan: double_angle is 0 .. 8");
    for (int p : {cfg.cts_pieces, cfg.stc_pieces})
        if (p < 2 || p > BOOTSTRAP_MAX_PIECES) throw std::invalid_argument("slim_bootstrap_plan: the piece counts lie in [2, 5]");
    if (Q < cfg.stc_pieces + 1) throw std::invalid_argument("slim_bootstrap_plan: SlotToCoeff needs a chain of pieces + 1 limbs");
    const double q0 = static_cast<double>(primes[0]);

    SlimBootstrapPlan pl{};
    pl.K = cfg.K;
    pl.degree = cfg.degree;
    pl.double_angle = cfg.double_angle;
    pl.cts_pieces = cfg.cts_pieces;
    pl.stc_pieces = cfg.stc_pieces;
    pl.in_level = cfg.stc_pieces;
    pl.cts_level = cfg.cts_level;
    pl.ratio = cfg.ratio;
    pl.phase = cfg.phase;
    pl.amplitude = cfg.amplitude;
    pl.offset = cfg.offset;
    if (pl.cts_level < 0 || pl.cts_level >= Q) throw std::invalid_argument("slim_bootstrap_plan: no such CoeffToSlot level");
    // P factors and the limb the real part drops; the polynomial and the double angles
    pl.eval_level = pl.cts_level - pl.cts_pieces - 1;
    pl.out_level = pl.eval_level - bootstrap_bit_length(cfg.degree) - cfg.double_angle;
    if (pl.out_level < 0)
        throw std::invalid_argument("slim_bootstrap_plan: too few levels (CoeffToSlot pieces + 1 + bit length of the degree + "
                                    "double angles, and one limb left)");
    // 1. SlotToCoeff takes the label from D at level P_stc to q_0 / ratio at level 0: no pre-multiplier
    const double back = std::pow(q0 / cfg.ratio / cfg.scale, 1.0 / pl.stc_pieces);
    double label = cfg.scale;
    for (int g = 0; g < pl.stc_pieces; g++) {
        const double q = static_cast<double>(primes[(size_t) (pl.in_level - g)]);
        pl.stc_scale[g] = back * q;
        label = label * pl.stc_scale[g] / q; // the product's label, then the rescale: as the sequence's caller labels it
        pl.stc_label[g] = label;
    }
    // 2. the raise
    pl.raise_scale = q0 * static_cast<double>(cfg.K);
    // 3. CoeffToSlot brings the label to the scale of the polynomial's input
    const double S = static_cast<double>(primes[(size_t) pl.eval_level]);
    const double share = std::pow(S / pl.raise_scale, 1.0 / pl.cts_pieces);
    label = pl.raise_scale;
    for (int f = 0; f < pl.cts_pieces; f++) {
        const double q = static_cast<double>(primes[(size_t) (pl.cts_level - f)]);
        pl.cts_scale[f] = share * q;
        label = label * pl.cts_scale[f] / q;
        pl.cts_label[f] = label;
    }
    // 4. one plan from the label as it comes out
    pl.eval_in_scale = label;
    pl.eval_target_scale = S;
    const std::vector<PolyStep> steps = eval_trig_plan(cfg.K, cfg.degree, cfg.double_angle, cfg.phase, cfg.amplitude, cfg.offset,
                                                       pl.eval_level, pl.eval_in_scale, pl.eval_target_scale, primes);
    if (steps.back().level != pl.out_level) throw std::invalid_argument("slim_bootstrap_plan: the plan does not end at its level");
    pl.eval_out_scale = steps.back().scale;
    // 5. the arithmetic value sin(2 pi z / rho) / 2 pi becomes (rho / 2 pi) sin(2 pi z / rho) by its label alone
    pl.out_scale = cfg.arithmetic ? pl.eval_out_scale / cfg.ratio : pl.eval_out_scale;
    for (int i = 0; i < BOOTSTRAP_MAX_PIECES; i++) {
        if (i < pl.cts_pieces && !(bootstrap_scale_ok(pl.cts_scale[i]) && pl.cts_scale[i] >= 1.0))
            throw std::invalid_argument("slim_bootstrap_plan: a CoeffToSlot factor's scale is below one or not finite");
        if (i < pl.stc_pieces && !(bootstrap_scale_ok(pl.stc_scale[i]) && pl.stc_scale[i] >= 1.0))
            throw std::invalid_argument("slim_bootstrap_plan: a SlotToCoeff factor's scale is below one or not finite");
    }
    if (!bootstrap_scale_ok(pl.out_scale)) throw std::invalid_argument("slim_bootstrap_plan: a scale left the range of a double");
    return pl;
}

} // namespace host
} // namespace hegpu
