// poly_eval.cpp -- see poly_eval.hpp.  Every function below names the reference function it restates; the arithmetic on
// scales is the reference's, operation for operation, so that the scales agree to the last bits.
#include "poly_eval.hpp"

#include <cmath>
#include <map>
#include <stdexcept>

namespace hegpu {
namespace host {

using cplx = std::complex<double>;

namespace {

int bit_length(int v)
{
    int b = 0;
    while (v > 0) { b++; v >>= 1; }
    return b;
}
int ceil_log2(int v) { return v <= 1 ? 0 : bit_length(v - 1); } // std::ceil(std::log2(v)) for v >= 1

// ckks/operator.cu:4615-4627
int optimal_split(int log_degree)
{
    int log_split = log_degree >> 1;
    const int a = (1 << log_split) + (1 << (log_degree - log_split)) + log_degree - log_split - 3;
    const int b = (1 << (log_split + 1)) + (1 << (log_degree - log_split - 1)) + log_degree - log_split - 4;
    if (a > b) log_split++;
    return log_split;
}

struct Poly {
    std::vector<cplx> c;
    int max_deg;
    bool lead;
    int degree() const { return (int) c.size() - 1; }
};

struct Planner {
    int basis;
    double threshold; // of the conditional rescale of q
    const std::vector<uint64_t>& primes;
    std::vector<PolyStep> steps;
    struct Reg { int level; double scale; };
    std::vector<Reg> regs;
    std::map<int, int> power; // power -> register

    double prime(int level) const
    {
        if (level < 0 || level >= (int) primes.size())
            throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
        return static_cast<double>(primes[(size_t) level]);
    }
    PolyStep& push(int kind, int level, double scale)
    {
        if (level < 0) throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
        if (!std::isfinite(scale) || scale <= 0) throw std::invalid_argument("poly_eval_plan: a scale left the range of a double");
        PolyStep s{};
        s.kind = kind;
        s.dst = (int) regs.size();
        s.a = s.b = -1;
        s.c = POLY_TAIL_NONE;
        s.level = level;
        s.mul_level = -1;
        s.scale = scale;
        for (int& r : s.term_reg) r = -1;
        regs.push_back({level, scale});
        steps.push_back(s);
        return steps.back();
    }

    // gen_power, :4292-4398
    void gen_power(int p)
    {
        if (power.count(p)) return;
        const bool pow2 = (p & (p - 1)) == 0;
        int a, b, c = 0;
        if (pow2) {
            a = b = p / 2;
        } else {
            const int k = ceil_log2(p) - 1;
            a = (1 << k) - 1;
            b = p + 1 - (1 << k);
            if (basis == POLY_CHEBYSHEV) c = std::abs(a - b);
        }
        gen_power(a);
        gen_power(b);
        if (c) gen_power(c); // the reference makes it after the product; the values are the same
        const Reg ra = regs[(size_t) power[a]], rb = regs[(size_t) power[b]];
        const int ml = ra.level < rb.level ? ra.level : rb.level;
        if (ml < 1) throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
        double scale = ra.scale * rb.scale;
        scale = scale / prime(ml);
        int level = ml - 1;
        int tail = POLY_TAIL_NONE;
        if (basis == POLY_CHEBYSHEV) {
            tail = POLY_TAIL_ONE;
            if (c) {
                tail = power[c];
                if (regs[(size_t) tail].level < level) level = regs[(size_t) tail].level;
            }
        }
        PolyStep& s = push(POLY_STEP_POWER, level, scale);
        s.a = power[a];
        s.b = power[b];
        s.c = tail;
        s.mul_level = ml;
        if (tail == POLY_TAIL_ONE) s.tail_const = scale;
        power[p] = s.dst;
    }

    // evaluate_poly_from_polynomial_basis, :4400-4484
    int leaf(double target_scale, int target_level, const Poly& pol)
    {
        const int degree = pol.degree();
        if (degree > POLY_LEAF_MAX) throw std::invalid_argument("poly_eval_plan: a leaf has more than 15 power terms");
        prime(target_level); // a level the chain has
        int level = target_level;
        for (int i = 1; i <= degree; i++) {
            const int l = regs[(size_t) power.at(i)].level;
            if (l < level) level = l;
        }
        PolyStep& s = push(POLY_STEP_LEAF, level, target_scale);
        s.w0[0] = std::round(pol.c[0].real() * target_scale);
        s.w0[1] = std::round(pol.c[0].imag() * target_scale);
        for (int i = 1; i <= degree; i++) {
            const int r = power.at(i);
            const double ratio = target_scale / regs[(size_t) r].scale;
            const double re = std::round(pol.c[(size_t) i].real() * ratio), im = std::round(pol.c[(size_t) i].imag() * ratio);
            if (!std::isfinite(re) || !std::isfinite(im))
                throw std::invalid_argument("poly_eval_plan: a weight left the range of a double");
            if (re == 0 && im == 0) continue;
            s.term_reg[s.n_terms] = r;
            s.w[s.n_terms][0] = re;
            s.w[s.n_terms][1] = im;
            s.n_terms++;
        }
        if (!std::isfinite(s.w0[0]) || !std::isfinite(s.w0[1]))
            throw std::invalid_argument("poly_eval_plan: a weight left the range of a double");
        return s.dst;
    }

    // Polynomial::split_coeffs, :6633-6678
    static void split_coeffs(const Poly& p, int split, int basis, Poly& q, Poly& r)
    {
        const int degree = p.degree();
        r.max_deg = split - 1;
        if (p.max_deg != degree) r.max_deg = p.max_deg - (degree - split + 1);
        r.c.assign(p.c.begin(), p.c.begin() + split);
        r.lead = false;
        q.c.assign((size_t) (degree - split + 1), p.c[(size_t) split]);
        if (basis == POLY_MONOMIAL) {
            for (int i = split + 1; i <= degree; i++) q.c[(size_t) (i - split)] = p.c[(size_t) i];
        } else {
            for (int i = split + 1, j = 1; i <= degree; i++, j++) {
                q.c[(size_t) (i - split)] = cplx(2.0, 0.0) * p.c[(size_t) i];
                r.c[(size_t) (split - j)] = r.c[(size_t) (split - j)] - p.c[(size_t) i];
            }
        }
        q.max_deg = p.max_deg;
        q.lead = p.lead;
    }

    // evaluate_poly_recurse, :4486-4613
    int recurse(int target_level, double target_scale, const Poly& pol, int log_split)
    {
        const int degree = pol.degree();
        const int split = 1 << log_split;
        if (degree < split) {
            if (pol.lead && log_split > 1 && degree > 0 && (pol.max_deg % (1 << (log_split + 1)) > (1 << (log_split - 1))))
                return recurse(target_level, target_scale, pol, ceil_log2(degree) >> 1);
            if (pol.lead) target_scale = target_scale * prime(target_level);
            return leaf(target_scale, target_level, pol);
        }
        int next_power = split;
        while (next_power < (degree >> 1) + 1) next_power <<= 1;
        Poly q, r;
        split_coeffs(pol, next_power, basis, q, r);
        const double current_qi = !pol.lead ? prime(target_level + 1) : prime(target_level);
        const int g = power.at(next_power);
        const double next_target_scale = target_scale * current_qi / regs[(size_t) g].scale;
        const int rq = recurse(target_level + 1, next_target_scale, q, log_split);
        Reg cur = regs[(size_t) rq];
        int rescale_first = 0;
        if (cur.scale >= threshold) { // :4545
            if (cur.level < 1) throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
            cur.scale = cur.scale / prime(cur.level);
            cur.level -= 1;
            rescale_first = 1;
        }
        const int ml = cur.level < regs[(size_t) g].level ? cur.level : regs[(size_t) g].level;
        const double scale = cur.scale * regs[(size_t) g].scale;
        const int rr = recurse(ml, scale, r, log_split);
        const int level = ml < regs[(size_t) rr].level ? ml : regs[(size_t) rr].level;
        PolyStep& s = push(POLY_STEP_COMBINE, level, scale);
        s.a = rq;
        s.b = g;
        s.c = rr;
        s.mul_level = ml;
        s.rescale_first = rescale_first;
        return s.dst;
    }
};

} // namespace

std::vector<PolyStep> poly_eval_plan(int basis, const std::vector<cplx>& coeffs, int max_deg, bool lead, int level,
                                     double scale, double target_scale, const std::vector<uint64_t>& primes)
{
    if (basis != POLY_MONOMIAL && basis != POLY_CHEBYSHEV) throw std::invalid_argument("poly_eval_plan: unknown basis");
    const int degree = (int) coeffs.size() - 1;
    if (degree < 2) throw std::invalid_argument("poly_eval_plan: the degree is at least 2");
    if (degree >= (1 << 20)) throw std::invalid_argument("poly_eval_plan: the degree is below 2^20");
    if (max_deg < degree) throw std::invalid_argument("poly_eval_plan: max_deg is at least the degree");
    for (const cplx& c : coeffs)
        if (!std::isfinite(c.real()) || !std::isfinite(c.imag()))
            throw std::invalid_argument("poly_eval_plan: a coefficient is not a finite number");
    if (!std::isfinite(scale) || !std::isfinite(target_scale) || scale <= 0 || target_scale <= 0)
        throw std::invalid_argument("poly_eval_plan: a scale is not a positive finite number");
    if (level < 0 || level >= (int) primes.size()) throw std::invalid_argument("poly_eval_plan: no such level");
    for (uint64_t p : primes)
        if (p < 2) throw std::invalid_argument("poly_eval_plan: a prime below 2");

    Planner pl{basis, target_scale / 2, primes, {}, {}, {}};
    pl.regs.push_back({level, scale});
    pl.power[1] = 0;
    // evaluate_poly, :4629-4671
    const int log_degree = bit_length(degree);
    const int log_split = optimal_split(log_degree);
    if ((1 << log_split) - 1 > POLY_LEAF_MAX) throw std::invalid_argument("poly_eval_plan: a leaf has more than 15 power terms");
    for (int p = (1 << log_split) - 1; p >= 1; p--) pl.gen_power(p);
    for (int i = log_split; i < log_degree; i++) pl.gen_power(1 << i);
    const int initial_target_level = level - log_degree + 1;
    if (initial_target_level < 0) throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
    const Poly top{coeffs, max_deg, lead};
    pl.recurse(initial_target_level, target_scale, top, log_split);
    PolyStep& last = pl.steps.back();
    if (last.scale / pl.prime(last.level) >= target_scale / 2.0) { // :4664-4668
        if (last.level < 1) throw std::invalid_argument("poly_eval_plan: too few levels for the polynomial's depth");
        last.scale = last.scale / pl.prime(last.level);
        last.level -= 1;
        last.rescale_after = 1;
    }
    return pl.steps;
}

// eval_mod, ckks/operator.cu:4248-4290: the polynomial, then r times (square, relinearize, double, subtract, rescale).
// One cosine with a phase, an amplitude and an offset; EvalMod is (1/4, 1 / 2 pi, 0).
std::vector<PolyStep> eval_trig_plan(int K, int degree, int double_angle, double phase, double amplitude, double offset,
                                     int level, double scale, double target_scale, const std::vector<uint64_t>& primes)
{
    const int r = double_angle;
    if (K < 1 || K > (1 << 20)) throw std::invalid_argument("eval_mod_plan: K is at least 1");
    if (r < 0 || r > 8) throw std::invalid_argument("eval_mod_plan: double_angle is 0 .. 8");
    if (degree < 2 || degree > 255) throw std::invalid_argument("eval_mod_plan: the degree is 2 .. 255");
    if (!std::isfinite(scale) || !std::isfinite(target_scale) || scale <= 0 || target_scale <= 0)
        throw std::invalid_argument("eval_mod_plan: a scale is not a positive finite number");
    if (!std::isfinite(phase) || !std::isfinite(amplitude) || !std::isfinite(offset) || !(amplitude > 0))
        throw std::invalid_argument("eval_trig_plan: phase and offset are finite, the amplitude is positive and finite");
    if (level < 0 || level >= (int) primes.size()) throw std::invalid_argument("eval_mod_plan: no such level");
    for (uint64_t p : primes)
        if (p < 2) throw std::invalid_argument("eval_mod_plan: a prime below 2");
    const int level_p = level - bit_length(degree); // where the evaluator leaves the interpolant
    if (level_p - r < 0) throw std::invalid_argument("eval_mod_plan: too few levels for the polynomial's depth and the double angles");
    // the square-root chain (:4257-4265): the scale p must have for the r squarings to end at target_scale
    double target_p = target_scale;
    for (int i = 0; i < r; i++) target_p = std::sqrt(target_p * static_cast<double>(primes[(size_t) (level_p - r + i + 1)]));
    // Chebyshev interpolant of g(u) = c cos(2 pi (K u - phase) / 2^r) at the degree + 1 Chebyshev nodes
    const double pi = 3.14159265358979323846;
    const double c = std::pow(amplitude, 1.0 / static_cast<double>(1 << r));
    const int m = degree + 1;
    std::vector<double> g((size_t) m);
    for (int j = 0; j < m; j++) {
        const double u = std::cos(pi * (j + 0.5) / m);
        g[(size_t) j] = c * std::cos(2.0 * pi * (K * u - phase) / static_cast<double>(1 << r));
    }
    std::vector<cplx> coeffs((size_t) m);
    for (int k = 0; k < m; k++) {
        double s = 0;
        for (int j = 0; j < m; j++) s += g[(size_t) j] * std::cos(pi * k * (j + 0.5) / m);
        coeffs[(size_t) k] = cplx(s * (k ? 2.0 : 1.0) / m, 0.0);
    }
    if (r == 0 && offset != 0) coeffs[0] += offset; // no double angle to carry it: the offset is the polynomial's
    std::vector<PolyStep> steps = poly_eval_plan(POLY_CHEBYSHEV, coeffs, degree, true, level, scale, target_p, primes);
    if (steps.back().level != level_p) throw std::invalid_argument("eval_mod_plan: the interpolant does not end at its level");
    // y <- 2 y^2 - c^(2^(i+1)): a POWER step whose tail is the constant at the step's scale; the last one leaves the offset
    double cc = c;
    for (int i = 0; i < r; i++) {
        const PolyStep prev = steps.back();
        cc *= cc;
        PolyStep s{};
        s.kind = POLY_STEP_POWER;
        s.dst = (int) steps.size() + 1;
        s.a = s.b = prev.dst;
        s.c = POLY_TAIL_ONE;
        s.mul_level = prev.level;
        s.level = prev.level - 1;
        s.scale = prev.scale * prev.scale / static_cast<double>(primes[(size_t) prev.level]);
        s.tail_const = ((i == r - 1 && offset != 0) ? cc - offset : cc) * s.scale;
        for (int& t : s.term_reg) t = -1;
        if (!std::isfinite(s.scale) || !(std::fabs(s.tail_const) < 3.4e38))
            throw std::invalid_argument("eval_mod_plan: a scale left the range of the evaluator");
        steps.push_back(s);
    }
    return steps;
}

std::vector<PolyStep> eval_mod_plan(int K, int degree, int double_angle, int level, double scale, double target_scale,
                                    const std::vector<uint64_t>& primes)
{
    const double pi = 3.14159265358979323846;
    return eval_trig_plan(K, degree, double_angle, 0.25, 1.0 / (2.0 * pi), 0.0, level, scale, target_scale, primes);
}

} // namespace host
} // namespace hegpu
