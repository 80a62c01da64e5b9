// encoding_transform.hpp -- host only: the factors of the CKKS encoder's special FFT, in diagonal form, for
// CoeffToSlot / SlotToCoeff.  No device, no context: FP64 on the host.
//
// n = N/2 slots, L = log2 n, zeta = exp(2 pi i / 2N).  The slot vector of a polynomial with real coefficients a is
// z = U w, w_k = a_k + i a_{k+n}, U[j][k] = zeta^(5^j k), and U = F_L ... F_1 B with B the bit reversal on L bits and
// F_s the radix-2 butterfly stage of length len = 2^s, h = len/2: row i+j = (1 at i+j, w at i+j+h), row i+j+h =
// (1 at i+j, -w at i+j+h), w = zeta^((5^j mod 4 len) 2N / (4 len)).
//
// The L stages are split into `pieces` groups of floor(L/pieces) or ceil(L/pieces) consecutive stages, the larger groups
// applied first.  forward (SlotToCoeff): group 0 holds stage 1; piece p is F_{s+g} ... F_{s+1}.  inverse (CoeffToSlot):
// group 0 holds stage L; piece p is F_{s+1}^-1 ... F_{s+g}^-1 times 2^(-1/pieces), so that all pieces together give
// 1/2 B U^-1 (the half of x + conj x and -i (x - conj x)).  A piece over stages s+1 .. s+g has the stride 2^s: every
// offset of a non-zero diagonal is a multiple of it, and there are at most 2^(g+1) - 1 of them.
#pragma once
#include <complex>
#include <vector>

namespace hegpu {
namespace host {

struct EncodingTransformPiece {
    int first_stage = 0, stages = 0, stride = 0; // stages first_stage .. first_stage + stages - 1; stride = 2^(first_stage-1)
    std::vector<int> offsets;                    // signed, in (-n/2, n/2], ascending
    std::vector<std::vector<std::complex<double>>> diags; // per offset k: diag_k[t] = M[t][(t + k) mod n], n values
};

// group `piece` (0 = applied first) of the split into `pieces` groups; std::invalid_argument for n_power outside
// [2, 17], pieces outside [2, 5] or more pieces than stages, piece outside [0, pieces)
EncodingTransformPiece encoding_transform_piece(int n_power, bool inverse, int pieces, int piece);

// The chain of a transform's giant steps: a Horner fold over the signed shifts.  Each of the n2 shifts,
// given in [0, slots), is taken as its signed representative in (-slots/2, slots/2].  The non-negative ones, ascending,
// each have the one before as parent; the negative ones, from the one nearest zero outwards, likewise, and the first of
// them hangs on the zero shift if there is one.  parent[j] = -1: a root.  link_shifts[j] in [0, slots): term j's signed
// shift minus its parent's (a root's own shift), the rotation of op_ckks_linear_transform's link j.  The rotations a term
// meets on its way to the result add up to its own shift, so the pre-rotated diagonals of the direct plan stay valid, and
// giant steps that are dense on both sides of zero -- the groups of the special FFT -- need two distinct links.
// std::invalid_argument: n2 outside [1, 16], slots no power of two, a shift outside [0, slots), a null argument.
void giant_step_chain(const int* giant_shifts, int n2, int slots, int* parent, int* link_shifts);

} // namespace host
} // namespace hegpu
