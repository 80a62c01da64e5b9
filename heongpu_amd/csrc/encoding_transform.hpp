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

} // namespace host
} // namespace hegpu
