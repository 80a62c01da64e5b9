// encoding_transform.cpp -- see encoding_transform.hpp.  Matrices are kept as maps offset -> diagonal throughout: a
// dense n x n matrix is 8 GB at N = 2^16, a group of five stages is 63 diagonals of n values.
#include "encoding_transform.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>

namespace hegpu {
namespace host {

using cplx = std::complex<double>;
using DiagMatrix = std::map<int, std::vector<cplx>>; // offset in [0, n) -> diag_k[t] = M[t][(t + k) mod n]

// F_s (or its inverse) for n slots; two_n = 2N
static DiagMatrix stage_matrix(int n, int s, bool inverse)
{
    const int len = 1 << s, h = len >> 1;
    const long two_n = 4L * n;
    const double pi = std::acos(-1.0);
    std::vector<cplx> w((size_t) h); // the twiddle of butterfly j
    long pow5 = 1;
    for (int j = 0; j < h; j++) {
        const long e = (pow5 * (two_n / (4L * len))) % two_n;
        const double a = 2.0 * pi * (double) e / (double) two_n;
        w[(size_t) j] = cplx(std::cos(a), std::sin(a));
        pow5 = (pow5 * 5) % (4L * len);
    }
    DiagMatrix m;
    auto diag = [&](int k) -> std::vector<cplx>& {
        auto it = m.find(k);
        if (it == m.end()) it = m.emplace(k, std::vector<cplx>((size_t) n, cplx(0, 0))).first;
        return it->second;
    };
    const int up = h % n, down = (n - h) % n; // the last stage has up == down == n/2
    for (int t = 0; t < n; t++) {
        const int pos = t & (len - 1), j = pos & (h - 1);
        const bool top = pos < h;
        if (!inverse) { // rows (1, w) and (1, -w)
            if (top) {
                diag(0)[(size_t) t] += 1.0;
                diag(up)[(size_t) t] += w[(size_t) j];
            } else {
                diag(down)[(size_t) t] += 1.0;
                diag(0)[(size_t) t] += -w[(size_t) j];
            }
        } else { // the inverse: rows 1/2 (1, 1) and 1/2 (conj w, -conj w)
            if (top) {
                diag(0)[(size_t) t] += 0.5;
                diag(up)[(size_t) t] += 0.5;
            } else {
                diag(down)[(size_t) t] += 0.5 * std::conj(w[(size_t) j]);
                diag(0)[(size_t) t] += -0.5 * std::conj(w[(size_t) j]);
            }
        }
    }
    return m;
}

// C = A B in diagonal form: c_{a+b}[t] += a_a[t] b_b[(t + a) mod n]
static DiagMatrix multiply(const DiagMatrix& A, const DiagMatrix& B, int n)
{
    DiagMatrix C;
    for (const auto& a : A)
        for (const auto& b : B) {
            const int k = (a.first + b.first) % n;
            auto it = C.find(k);
            if (it == C.end()) it = C.emplace(k, std::vector<cplx>((size_t) n, cplx(0, 0))).first;
            std::vector<cplx>& c = it->second;
            for (int t = 0; t < n; t++) c[(size_t) t] += a.second[(size_t) t] * b.second[(size_t) ((t + a.first) & (n - 1))];
        }
    return C;
}

EncodingTransformPiece encoding_transform_piece(int n_power, bool inverse, int pieces, int piece)
{
    if (n_power < 2 || n_power > 17) throw std::invalid_argument("encoding transform: log2 N lies in [2, 17]");
    if (pieces < 2 || pieces > 5) throw std::invalid_argument("encoding transform: the piece count lies in [2, 5]");
    const int L = n_power - 1, n = 1 << L;
    if (pieces > L) throw std::invalid_argument("encoding transform: more pieces than FFT stages");
    if (piece < 0 || piece >= pieces) throw std::invalid_argument("encoding transform: no such piece");
    // group sizes in the order of application: the L mod pieces larger ones first
    int before = 0, g = 0;
    for (int p = 0; p <= piece; p++) {
        before += g;
        g = L / pieces + (p < L % pieces ? 1 : 0);
    }
    EncodingTransformPiece out;
    out.stages = g;
    out.first_stage = inverse ? L - before - g + 1 : before + 1; // forward starts at stage 1, inverse at stage L
    out.stride = 1 << (out.first_stage - 1);
    // forward: F_{s+g} ... F_{s+1}, a later stage goes on the left; inverse: F_{s+1}^-1 ... F_{s+g}^-1, on the right
    DiagMatrix m = stage_matrix(n, out.first_stage, inverse);
    for (int s = out.first_stage + 1; s < out.first_stage + g; s++) {
        const DiagMatrix f = stage_matrix(n, s, inverse);
        m = inverse ? multiply(m, f, n) : multiply(f, m, n);
    }
    if (inverse) {
        const double share = std::pow(2.0, -1.0 / pieces); // the half of the real / imaginary split, spread evenly
        for (auto& d : m)
            for (cplx& v : d.second) v *= share;
    }
    std::map<int, const std::vector<cplx>*> by_signed; // (-n/2, n/2], ascending
    for (const auto& d : m) by_signed[d.first > n / 2 ? d.first - n : d.first] = &d.second;
    for (const auto& d : by_signed) {
        out.offsets.push_back(d.first);
        out.diags.push_back(*d.second);
    }
    return out;
}

void giant_step_chain(const int* giant_shifts, int n2, int slots, int* parent, int* link_shifts)
{
    if (!giant_shifts || !parent || !link_shifts) throw std::invalid_argument("giant_step_chain: null argument");
    if (n2 < 1 || n2 > 16) throw std::invalid_argument("giant_step_chain: n2 lies in [1, 16]");
    if (slots < 1 || (slots & (slots - 1))) throw std::invalid_argument("giant_step_chain: the slot count is a power of two");
    std::vector<std::pair<int, int>> order; // (signed shift, term)
    for (int j = 0; j < n2; j++) {
        const int s = giant_shifts[j];
        if (s < 0 || s >= slots) throw std::invalid_argument("giant_step_chain: a shift outside [0, slots)");
        order.emplace_back(s > slots / 2 ? s - slots : s, j);
    }
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    size_t first = 0; // the first non-negative shift
    while (first < order.size() && order[first].first < 0) first++;
    auto link = [&](size_t at, const std::pair<int, int>* to) {
        parent[order[at].second] = to ? to->second : -1;
        link_shifts[order[at].second] = ((order[at].first - (to ? to->first : 0)) % slots + slots) % slots;
    };
    for (size_t at = first; at < order.size(); at++) link(at, at > first ? &order[at - 1] : nullptr);
    const bool zero = first < order.size() && order[first].first == 0;
    for (size_t at = first; at-- > 0;) link(at, at + 1 < first ? &order[at + 1] : zero ? &order[first] : nullptr);
}

} // namespace host
} // namespace hegpu
