// context.hpp -- parameter set + device-resident tables of one HE context.
//
// Host-side counterpart of the reference's HEContextImpl<BFV|CKKS>::generate()
// (reference src/lib/host/ckks/context.cu:272-440, bfv/context.cu:396-705):
// prime chain, psi, NTT tables, mod-down / rescale constants, the CKKS order
// tables (ckks/operator.cu:24-56) and the BFV BEHZ constants
// (bfv/context.cu:939-1347).  Host tables are kept under the reference's
// member names so tests can compare them one by one.
#pragma once
#include "modarith.cuh"
#include "ntt.hpp"
#include "rns.hpp"
#include <map>
#include <string>
#include "drbg.hpp"
#include <vector>

namespace hegpu {

// context.cpp: the value of an environment variable that holds a whole decimal integer (false otherwise)
bool env_long(const char* name, long* out);


enum Scheme { SCHEME_BFV = 1, SCHEME_CKKS = 2 };

// Offset of row `depth` in a triangular per-depth table whose rows hold first, first - 1, ... entries
// (reference ckks/operator.cu:949-955, 1181-1187)
inline int triangle_offset(int first, int depth)
{
    int location = 0;
    for (int i = 0; i < depth; i++) location += first - i;
    return location;
}

struct NttPlan {
    // device arrays, one entry / table per modulus
    Mod* mods = nullptr;
    ulonglong2* tw = nullptr;
    ulonglong2* itw = nullptr;
    ulonglong2* twB = nullptr;  // row-pass last-four-stages layout (see ntt.hpp)
    ulonglong2* itwB = nullptr;
    double* twB8 = nullptr;     // twB's layout as plain doubles (FP64 moduli; zeros elsewhere): 8 bytes per twiddle for the row pass
    ulonglong2* ninv = nullptr;
    ulonglong2* w1ninv = nullptr;
    int count = 0;
    int has_fp = 0, has_int = 0; // moduli on the FP64 / on the integer butterflies
    std::vector<unsigned char> fp; // host copy of Mod::fp per modulus
    std::vector<unsigned char> bits; // host copy of Mod::bit per modulus
    // integer butterflies: moduli up to this run the whole forward transform correction-free (NttArgs::lazy_q_max)
    u64 lazy_q_max = 0;
};

// Device copies of the host tables that upload() files under the same names (context.cpp, the row table in upload();
// the BFV BEHZ tables go straight into BehzDev).  A member is null where build_host() makes no such table: the groups
// say when it does, which is the check that an entry point (cabi.cpp) makes before a sequence reads the member.
struct DevTables {
    // every context
    const u64 *psi_half, *last_q_modinv, *half, *half_mod, *factor;
    // P_size > 1 (key-switching method II)
    const u64 *m2_md_W0, *m2_md_G, *m2_md_C, *m2_Mi_inv, *m2_matrix, *m2_prod, *m2_matrix_mg, *m2_negprod_mg;
    const int *m2_I_j, *m2_I_location;
    // CKKS (rescaled_*: empty with a single ciphertext prime, which has no rescale)
    const u64 *rescaled_last_q_modinv, *rescaled_half_mod, *rescaled_half;
    const u64* mod_raise_half_mod; // (q_0 + 1) / 2 modulo q_j, j < Q: the modulus raise as a load transform (ops.cpp)
    const u64 *Mi, *Mi_inv, *upper_half_threshold, *decryption_modulus, *special_fft_roots_table, *special_ifft_roots_table;
    const int *new_prime_locations, *new_input_locations, *reverse_order, *mpc_refresh_order;
    // BFV
    const u64 *coeff_div_plain_modulus, *upper_halfincrement, *Qi_t, *Qi_gamma, *Qi_inverse;
    // BFV with batching (plan_plain.count != 0)
    const int* encoding_location;
};

// Everything hegpu_context_clone copies: the parameter set, the host tables and the options.
struct ContextHost {
    int scheme = 0;
    int n_power = 0;
    u64 n = 0;
    int Q_size = 0, P_size = 0, Qp_size = 0;
    int bsk_size = 0;
    u64 plain_modulus = 0;
    std::vector<u64> primes; // Q then P
    std::map<std::string, std::vector<u64>> host; // named host tables: read by build_host(), upload() and hegpu_context_get only
    // the host values the operator sequences read on every call (build_host())
    struct HostVals {
        u64 half = 0;                         // half[0]
        std::vector<u64> rescaled_half;       // CKKS, per depth
        u64 mod_raise_half = 0;               // CKKS: (q_0 + 1) / 2
        std::vector<u64> new_prime_locations; // CKKS: host copy of the device table (ops.cpp: fill_int_slots)
        // BFV
        u64 Q_mod_t = 0, upper_threshold = 0, gamma = 0, mulq_inv_t = 0, mulq_inv_gamma = 0, inv_gamma = 0;
        u64 inv_prod_q_mod_m_tilde = 0, inv_prod_B_mod_m_sk = 0;
    } hv;
    // key-switching method II (P_size > 1): per-depth digit partition + table
    // offsets into the flattened host/device arrays "m2_*"
    struct M2Level {
        int d = 0, rc = 0;
        int off_digits = 0; // into m2_I_j / m2_I_location
        int off_mi = 0;     // into m2_Mi_inv
        int off_matrix = 0; // into m2_matrix
        int off_prod = 0;   // into m2_prod
    };
    std::vector<M2Level> m2_levels;
    int m2_width = 0; // digit width m: 2 for BFV, P_size for CKKS
    // ---- options: one row each in context.cpp (kOptions: name, HEGPU_<NAME> variable that seeds the default when a
    // context is created, range, rule); hegpu_context_set_option (include/hegpu.h) is the interface
    int fused_row_mac = -1;    // 1 / 0 force the fused / the reference's key-switch sequence, otherwise by launch size (ops.cpp: use_fused_row_mac)
    bool fused_moddown = true; // 0: separate stage-two kernel
    int col_multi = -1;        // form of the decomposing column pass (NttArgs::col_multi)
    int single_pass = -1;      // 1 / 0 force the single pass / the two passes for N <= 2^14, otherwise by launch size (NttArgs::single_pass)
    bool ntt_galois = true;    // 0: CKKS rotations in the reference's order (permutation in the coefficient domain)
    bool galois_scatter = true; // 0: the NTT-domain permutation as a kernel of its own (gather) instead of the mod-down epilogue's store
    int digit_split = -1;      // 0 never, 2 / 4 always that many workgroups per fused key-switch unit, -1 by launch size
    bool copy_along = true;    // 0: the rescale's copy of the kept limbs always has its own launch
    bool fuse_inverse = true;  // 0: the INTT feeding a decomposing launch runs on its own
    bool moddown_in_mac = true; // 0: CKKS method I, fused key switch: the mod-down row pass as a launch of its own instead of the inner product's tail
    bool wide_access = true;   // 0: fused key switch without digit splits: the row pass + inner product in the natural ownership, 8-byte global accesses (KsMacArgs::wide)
    bool fused_tensor = true;  // BFV multiply: the tensor product as the load transform of the inverse transform (0: its own kernel)
    bool fp_ntt = true;        // 0: every modulus on the integer butterflies (read when the tables are built)
    int behz_split = -1;       // BFV BEHZ kernels: rows over four wavefronts (1), one thread per coefficient (0), by launch size (-1)
};

struct Context : ContextHost {
    void seed_options_from_env();
    // 0 ok, 1 unknown name, 2 value out of range, 3 too late (the tables are already on the device)
    int set_option(const char* name, int value);
    int get_option(const char* name, int* value) const;
    GaussCdt gauss_cdt{}; // rounded Gaussian, sigma = 3.2 (drbg.hpp)

    // ---- device state (valid after upload())
    bool uploaded = false;
    int device = -1;
    NttPlan plan_qp;    // tables for the Q' chain
    NttPlan plan_merge; // BFV: [q_0..q_{Q-1}, Bsk...]
    NttPlan plan_plain; // BFV batching: the plain modulus t alone (bfv/context.cu:489-499), when 2N | t-1
    std::map<std::string, void*> dev; // the device tables by name: owns them; read by hegpu_context_device_ptr only
    DevTables tab{};
    BehzDev behz{};

    ~Context();
    void build_host();           // derive every host table from `primes`
    hipError_t upload();         // allocate + copy device tables (current device)
    void release_device();

    NttArgs ntt_args(int table_set) const; // 0 = Q' chain, 1 = merged q|Bsk
    // the mod-down by the special primes of a ciphertext at `depth`; rescale (CKKS, depth < Q_size - 1): by its last prime
    ModDown moddown(int depth, bool rescale = false) const;
};

} // namespace hegpu
