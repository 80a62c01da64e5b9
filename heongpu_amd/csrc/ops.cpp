// ops.cpp -- operator sequences (the reference's host orchestration), batched
// over independent ciphertexts and free of allocation, on the device and on the
// host: all temporaries live in a caller-provided workspace and every table is a
// typed member of the context (Context::tab / hv, no lookup by name), so the
// sequences can be captured in a hipGraph.  The one exception is
// op_gen_secret_key, which stages its index list in a host vector and waits.
#include "ops.hpp"
#include <algorithm>
#include <vector>
#include <utility>

namespace hegpu {

#define TRY(x)                           \
    do {                                 \
        hipError_t e__ = (x);            \
        if (e__ != hipSuccess) return e__; \
    } while (0)

static u64 inv_mod_2n(u64 g, u64 two_n)
{
    // g odd, two_n a power of two: Newton iteration
    u64 x = g;
    for (int i = 0; i < 6; i++) x *= 2 - g * x;
    return x & (two_n - 1);
}

// The fused row pass + inner product runs one workgroup per (ciphertext, target modulus, 16-row tile) that walks
// all digits; a launch too small to fill the chip finishes sooner as the reference's sequence -- the transform of
// all digits x moduli as independent limbs, then the element-wise inner product.  512 workgroups of this kernel are
// resident at a time (two per CU); measured crossover (tools/relin_sweep.py, relinearize of B ciphertexts, fused
// against unfused): N = 2^14, Q = 8: beyond B = 16 (36 B workgroups); N = 2^15, Q = 15: B = 4 388 / 360 us, B = 8
// 609 / 685 (128 B); N = 2^16, Q = 16: B = 1 401 / 288, B = 2 476 / 452, B = 4 688 / 788 (272 B); Q = 30: B = 1
// 804 / 758, B = 2 1098 / 1194 (496 B) -- one and a half rounds of resident workgroups.  Chains of integer-butterfly
// moduli (the 58/59-bit default chains) cross earlier, their transforms being the larger part of either path:
// N = 2^15, Q = 14: B = 2 242 / 220, B = 4 361 / 377 (120 B); N = 2^16, Q = 14: B = 1 287 / 274, B = 2 388 / 426
// (240 B); Q = 29: B = 1 756 / 866 (480 B).
static long fused_row_mac_need(const Context& c)
{
    size_t fp = 0;
    for (unsigned char f : c.plan_qp.fp) fp += f ? 1 : 0;
    return (2 * fp > c.plan_qp.fp.size()) ? 768 : 400;
}
// Between the two: the fused kernel with 2 (or, forced, 4) workgroups per (ciphertext, limb slot, tile), each over a
// part of the digits, and a pass that adds the partial sums (KsMacArgs::splits).  Measured (tools/relin_sweep.py,
// us per launch, unfused / fused / two pieces / four pieces): N = 2^16, Q = 16: B = 1 289 / 368 / 307 / 289, B = 2
// 456 / 457 / 410 / 410; Q = 30: B = 1 766 / 810 / 718 / 687, B = 2 1217 / 1123 / 1044 / 1027; N = 2^15, Q = 15: B = 1
// 154 / 251 / 195 / 171, B = 2 219 / 307 / 255 / 234; chains of integer-butterfly moduli: never ahead, and the order
// of fused and unfused changes from box to box there.  Round 3, with the integer and the FP64 moduli of a split
// launch in one grid (ks_row_mac_split; before, two half-empty grids one after the other): unfused / fused / four
// pieces, N = 2^16, Q = 16: B = 1 294 / 409 / 285, B = 2 467 / 476 / 409, B = 4 813 / 702 / 701; Q = 30: B = 1
// 806 / 832 / 690, B = 2 1277 / 1138 / 1029, B = 4 2283 / 1864 / 1829; N = 2^15, Q = 15: B = 1 155 / 252 / 154, B = 2
// 221 / 302 / 232, B = 4 370 / 394 / 347 (tools/relin_small.py).  So: four pieces, on FP64-path chains at N = 2^16,
// for launches below two rounds of the fused path's size that reach one round that way.  Returns 0 (no split) or
// the number of pieces.
static int fused_digit_splits(const Context& c, int rc, int digits, int batch)
{
    if (c.digit_split == 0) return 0;
    if (c.digit_split > 0) return digits >= 2 * c.digit_split ? c.digit_split : 0;
    if (c.fused_row_mac >= 0 || c.n_power < 16 || digits < 8) return 0;
    const long wgs = (long) batch * rc * (long) (c.n >> 12), need = fused_row_mac_need(c);
    return (need == 768 && wgs < 2 * need && 4 * wgs >= need) ? 4 : 0;
}
static bool use_fused_row_mac(const Context& c, int rc, int batch)
{
    if (c.fused_row_mac >= 0) return c.fused_row_mac != 0;
    return (long) batch * rc * (long) (c.n >> 12) >= fused_row_mac_need(c);
}
// Method I on the large-launch fused path: the mod-down runs as the tail of the fused row pass + inner product
// (Context::moddown_in_mac, see ckks_keyswitch_core).  `key` null: the accumulator comes from elsewhere (hoisted
// rotations).
static bool use_moddown_in_mac(const Context& c, const u64* key, int l, int rc, int batch)
{
    return c.moddown_in_mac && c.fused_moddown && key && c.P_size == 1 && use_fused_row_mac(c, rc, batch) &&
           !fused_digit_splits(c, rc, l, batch) && (long) 2 * l * batch <= 65535;
}

// The target slots of a decomposing launch over the Q' chain whose moduli run on the integer butterflies
// (NttArgs::int_slots).  `order`: host copy of the launch's mod_order (nullptr: slot k is modulus k).
static void fill_int_slots(const Context& c, NttArgs& a, const u64* order)
{
    int cnt = 0;
    for (int k = 0; k < a.decomp_mods; k++) {
        const int m = a.mod_offset + (order ? (int) order[k] : k);
        if (m < 0 || m >= (int) c.plan_qp.fp.size()) { a.int_slot_count = 0; return; }
        if (c.plan_qp.fp[m]) continue;
        if (cnt == 8) { a.int_slot_count = 0; return; } // more than the list holds: full grid
        a.int_slots[cnt++] = k;
    }
    a.int_slot_count = cnt ? cnt : -1;
}

// Bit length of the largest modulus on the integer butterflies among the target slots [slot_first, slot_first +
// slot_count) (0: all rc) of a key-switch launch at `depth`, 0 if it has none.  The slot order is read from the host
// copy of the table `order` points into (CKKS: new_prime_locations; null: slot k is modulus k); an order this does not
// know counts every integer modulus of the chain, which only makes the bound of ks_unreduced_exit more careful.
static int launch_int_q_bits(const Context& c, const int* order, int rc, int depth, int slot_first, int slot_count)
{
    const NttPlan& p = c.plan_qp;
    const u64* ho = nullptr;
    const size_t off = (size_t) triangle_offset(c.Qp_size, depth);
    if (order && order == c.tab.new_prime_locations + off && off + (size_t) rc <= c.hv.new_prime_locations.size())
        ho = c.hv.new_prime_locations.data() + off;
    int bits = 0;
    auto take = [&](size_t m) { if (m < p.bits.size() && !p.fp[m] && p.bits[m] > bits) bits = p.bits[m]; };
    if (order && !ho) {
        for (size_t m = 0; m < p.bits.size(); m++) take(m);
        return bits;
    }
    const int k0 = slot_count ? slot_first : 0, k1 = slot_count ? slot_first + slot_count : rc;
    for (int k = k0; k < k1; k++) take(ho ? (size_t) ho[k] : (size_t) k);
    return bits;
}

// Forward NTT of the key-switch digits followed by the inner product with the
// key.  `a` is the fully configured forward transform (plain or decomposing)
// whose output is [digits][rc][N] per ciphertext at a.out; the result
// [2][rc][N] goes to `acc`.  Fused path: column pass + ks_row_mac; otherwise
// two-pass NTT + rns_keyswitch_mac.
// `ident` (with a.skip_identity): the NTT-domain limbs [digits][N] of the
// polynomial being decomposed, `ident_stride` apart; digit d at modulus d is
// taken from there instead of being transformed.
// `which`: 1 = column pass only, 2 = row pass + inner product only, 3 = both (the measurement seam of
// hegpu_probe_ckks_relinearize; the unfused path ignores it)
// Fused path only: the row pass + inner product covers the limb slots [slot_first, slot_first + slot_count) (0: all),
// and `tail` (if not null) is the mod-down it ends with (KsMacArgs::tail, item pointers of the whole batch).
static hipError_t keyswitch_ntt_mac(const Context& c, NttArgs a, const u64* key, u64* acc, u64 acc_stride,
                                    int digits, int rc, int split, int level, const u64* ident, u64 ident_stride,
                                    int batch, hipStream_t st, int which = 3, int slot_first = 0, int slot_count = 0,
                                    const KsMacArgs::Tail* tail = nullptr)
{
    const int ppi = digits * rc;
    const int skip_identity = ident ? 1 : 0;
    a.skip_identity = skip_identity;
    const int splits = fused_digit_splits(c, rc, digits, batch);
    if (!splits && !use_fused_row_mac(c, rc, batch)) {
        if (slot_count || tail) return hipErrorInvalidValue;
        // identity digits (digit d at modulus d: the transform gives back the NTT-domain limb): copied instead of
        // transformed -- unless this path was chosen for a small launch, where one kernel less is worth more than
        // one transform in ten (same residues either way)
        if (ident && c.fused_row_mac == 0)
            TRY(rns_copy_diag(ident, ident_stride, a.out, a.out_item_stride, c.n_power, digits, rc, batch, st));
        else a.skip_identity = 0;
        TRY(ntt_launch(a, ppi * batch, false, st));
        return rns_keyswitch_mac(a.out, a.out_item_stride, key, acc, acc_stride, c.plan_qp.mods, c.n_power, digits, rc,
                                 c.Qp_size, split, level, batch, st);
    }
    const int chunk = 65535 / ppi; // gridDim.y limit of the column pass
    if (chunk < 1) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (batch - b0 < chunk) ? batch - b0 : chunk;
        NttArgs ca = a;
        ca.in = a.in + (u64) b0 * a.in_item_stride;
        ca.out = a.out + (u64) b0 * a.out_item_stride;
        if (which & 1) TRY(ntt_launch_fwd_col(ca, ppi * nb, st));
        if (!(which & 2)) continue;
        KsMacArgs k{};
        k.in = ca.out; k.in_item_stride = a.out_item_stride; k.key = key;
        k.out = acc + (u64) b0 * acc_stride; k.out_item_stride = acc_stride;
        k.mods = c.plan_qp.mods; k.tw = c.plan_qp.tw; k.twB = c.plan_qp.twB; k.twB8 = c.plan_qp.twB8; k.mod_order = a.mod_order;
        k.lazy_q_max = a.lazy_q_max; k.n_power = c.n_power; k.digits = digits; k.rc = rc; k.key_limbs = c.Qp_size; k.skip_identity = skip_identity;
        k.ident = ident ? ident + (u64) b0 * ident_stride : nullptr; k.ident_item_stride = ident_stride;
        k.splits = splits;
        k.wide = c.wide_access && splits <= 1;
        k.no_fp = !a.plan_has_fp;
        k.no_int = !a.plan_has_int || a.int_slot_count < 0;
        k.int_slot_count = a.int_slot_count > 0 ? a.int_slot_count : 0;
        for (int q = 0; q < 8; q++) k.int_slots[q] = a.int_slots[q];
        k.slot_first = slot_first; k.slot_count = slot_count;
        // the most digits one workgroup sums: all of them, or the largest range of a split launch (ks_index: d0, d1)
        k.unreduced_exit = ks_unreduced_exit(splits > 1 ? (digits + splits - 1) / splits : digits,
                                             launch_int_q_bits(c, a.mod_order, rc, level, slot_first, slot_count));
        if (slot_count && a.int_slot_count > 0) { // the integer slots of the range
            int cnt = 0;
            for (int q = 0; q < a.int_slot_count; q++)
                if (a.int_slots[q] >= slot_first && a.int_slots[q] < slot_first + slot_count) k.int_slots[cnt++] = a.int_slots[q];
            k.int_slot_count = cnt;
            k.no_int = cnt == 0;
            k.no_fp = k.no_fp || cnt == slot_count;
        }
        if (tail) {
            k.tail = *tail;
            k.tail.T += (u64) b0 * tail->T_item_stride;
            if (tail->ct) k.tail.ct += (u64) b0 * tail->ct_item_stride;
            k.tail.out += (u64) b0 * tail->out_item_stride;
        }
        TRY(ks_row_mac_launch(k, nb, st));
        if (splits > 1)
            TRY(rns_sum_partials(ca.out, a.out_item_stride, k.out, acc_stride, c.plan_qp.mods, a.mod_order, c.n_power,
                                 digits, rc, splits, nb, st));
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ workspace layouts
// Every workspace shape is stated once, here.  A layout holds the word offset of each region behind the first (which
// starts the workspace) and `per`, the words per item: the regions of a batch are `per` apart.  Composite layouts, whose
// regions are blocks of `batch` items, hold `total` instead.  The size queries return per * batch or total, the sequences
// take their pointers and strides from the same struct.  The sizes are public (callers allocate by them): where a row is
// larger than what its sequence touches, the slack stays and the layout says so.

// Key switch: [copy [2][l][N]] digits [l][rc][N] acc [accs][2][rc][N].  Relinearize has no copy; a rotation keeps the
// coefficient-domain ciphertext there; hoisted rotations take four accumulators when they have the room
// (OP_CKKS_ROTATE_HOISTED); BFV: depth 0, no copy.  Slack: method II fills d <= l of the digits.
struct KeySwitchWs { u64 digits, acc, acc_words, per; };
static KeySwitchWs keyswitch_ws(const Context& c, int depth, bool copy, int accs)
{
    const u64 l = c.Q_size - depth, rc = c.Qp_size - depth;
    const u64 digits = copy ? 2 * l * c.n : 0, acc = digits + l * rc * c.n, acc_words = 2 * rc * c.n;
    return {digits, acc, acc_words, acc + accs * acc_words};
}
int ops_rotate_hoisted_accumulators(const Context& c, int depth, int batch, size_t ws_elems)
{
    return ws_elems >= keyswitch_ws(c, depth, true, 4).per * (u64) batch ? 4 : 1;
}

// Two regions per item: where the second starts, and the words of both
struct PairWs { u64 second, per; };
// rescale: the dropped limb at every kept modulus [2][l-1][N], copy of the kept limbs (part stride l) [2][l][N]
static PairWs rescale_ws(const Context& c, int depth)
{
    const u64 l = c.Q_size - depth;
    return {2 * (l - 1) * c.n, (2 * (l - 1) + 2 * l) * c.n};
}
// modulus raise: the two q_0 limbs in the coefficient domain [2][N]
static u64 mod_raise_ws(const Context& c) { return 2 * c.n; }
// BFV multiply over the L = Q + bsk moduli: both operands extended [4][L][N], their tensor product [3][L][N]
static PairWs bfv_multiply_ws(const Context& c)
{
    const u64 L = c.Q_size + c.bsk_size;
    return {4 * L * c.n, (4 + 3) * L * c.n};
}
// CKKS decode: coefficient-domain copy [l][N], N/2 complex doubles [N]
static PairWs ckks_decode_ws(const Context& c, int depth) { const u64 l = c.Q_size - depth; return {l * c.n, (l + 1) * c.n}; }
// public key (share): e [Q'][N], a [Q'][N]
static PairWs public_key_share_ws(const Context& c) { return {(u64) c.Qp_size * c.n, (u64) 2 * c.Qp_size * c.n}; }
// switching key (share): e [errs][d][Q'][N], a [d][Q'][N]; errs = 2 in round 1 of the relinearisation key, whose round 2
// has the e region alone.  Slack: sized for Q digits, method II has d <= Q.
static PairWs switch_key_share_ws(const Context& c, int errs)
{
    return {(u64) errs * switch_key_digits(c) * c.Qp_size * c.n, (u64) (errs + 1) * c.Q_size * c.Qp_size * c.n};
}
// encryption of zero: u [Q'][N], e [2][Q'][N], pk * u [2][Q'][N]
struct EncryptWs { u64 e, pku, per; };
static EncryptWs encrypt_ws(const Context& c)
{
    const u64 limb = (u64) c.Qp_size * c.n;
    return {limb, 3 * limb, 5 * limb};
}
// BFV refresh merge: the rounded plaintexts [batch][N], the h0 sum of the head groups beyond 16 shares [batch][Q][N]
struct RefreshMergeWs { u64 head_sum, total; };
static RefreshMergeWs bfv_refresh_merge_ws(const Context& c, int batch)
{
    return {(u64) batch * c.n, (u64) (c.Q_size + 1) * c.n * batch};
}
// Logic gates: one three-part product per item (`ps` apart), then the largest workspace of the sequence -- CKKS:
// relinearize, rescale; BFV: multiply, relinearize, multiply-plain
struct GateWs { u64 ps, ks, total; };
static GateWs gate_ws(const Context& c, bool bfv, int depth, int batch)
{
    const auto row = [&](int op) { return ops_workspace_elems(c, op, bfv ? 0 : depth, batch); };
    const size_t most = bfv ? std::max({row(OP_BFV_MULTIPLY), row(OP_BFV_RELIN), row(OP_BFV_MULTIPLY_PLAIN)})
                            : std::max(row(OP_CKKS_RELIN), row(OP_CKKS_RESCALE));
    const u64 ps = (u64) 3 * (bfv ? c.Q_size : c.Q_size - depth) * c.n, ks = ps * batch;
    return {ps, ks, ks + most};
}

size_t ops_workspace_elems(const Context& c, int op, int depth, int batch)
{
    const u64 n = c.n;
    u64 per = 0;
    switch (op) {
        case OP_CKKS_RELIN: per = keyswitch_ws(c, depth, false, 1).per; break;
        case OP_CKKS_RESCALE: per = rescale_ws(c, depth).per; break;
        case OP_CKKS_GALOIS: per = keyswitch_ws(c, depth, true, 1).per; break;
        case OP_CKKS_ROTATE_HOISTED: per = keyswitch_ws(c, depth, true, 4).per; break;
        case OP_BFV_MULTIPLY: per = bfv_multiply_ws(c).per; break;
        case OP_BFV_RELIN:
        case OP_BFV_GALOIS: per = keyswitch_ws(c, 0, false, 1).per; break;
        case OP_KEYGEN_SECRET: per = n; break;                      // 2 x hamming weight ints
        case OP_KEYGEN_PUBLIC: per = public_key_share_ws(c).per; break;
        case OP_KEYGEN_SWITCH: per = switch_key_share_ws(c, 1).per; break;
        case OP_CKKS_ENCRYPT:
        case OP_BFV_ENCRYPT: per = encrypt_ws(c).per; break;
        case OP_BFV_DECRYPT: per = (u64) c.Q_size * n; break;        // c1*s
        case OP_BFV_DECODE: per = n; break;
        case OP_BFV_MULTIPLY_PLAIN: per = (u64) c.Q_size * n; break; // lifted + transformed plaintext
        case OP_CKKS_ENCODE: per = n; break;                         // N/2 complex doubles
        case OP_CKKS_DECODE: per = ckks_decode_ws(c, depth).per; break;
        case OP_MPC_KEY_SHARE: per = switch_key_share_ws(c, 2).per; break; // round 1 of the relinearisation key, the largest
        case OP_MPC_BFV_DECRYPT_MERGE: per = (u64) c.Q_size * n; break; // c0 + the shares beyond the first group
        case OP_MPC_REFRESH_SHARE: per = 0; break;                   // the noise is sampled and transformed in the share itself
        case OP_MPC_REFRESH_MERGE:                                   // CKKS: t = c0 + sum h0, [l][N] per item
            if (c.scheme != SCHEME_CKKS) return bfv_refresh_merge_ws(c, batch).total;
            per = (u64) (c.Q_size - depth) * n;
            break;
        case OP_CKKS_MOD_RAISE: per = mod_raise_ws(c); break;          // the same at every output depth
        case OP_CKKS_BOOTSTRAP: per = 3 * mod_raise_ws(c); break;      // the head of the refresh's workspace (bootstrap_head_ws)
        case OP_CKKS_LOGIC_GATE: return gate_ws(c, false, depth, batch).total;
        case OP_BFV_LOGIC_GATE: return gate_ws(c, true, depth, batch).total;
        default: return 0;
    }
    return per * (u64) batch;
}

hipError_t op_ckks_multiply(const Context& c, const u64* ct1, u64 s1, const u64* ct2, u64 s2, u64* out, u64 so,
                            int depth, int batch, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    return rns_cross_multiplication(ct1, s1, ct2, s2, out, so, c.plan_qp.mods, c.n_power, c.Q_size - depth, batch,
                                    st);
}

// Key switch (method I) of one NTT-domain polynomial per item, the shared core of relinearize and rotate
// (reference ckks/operator.cu:919-1020 and :1461-1545):
//   out[part p] = moddown(sum_i digit_i(src) * key[i][p]) + (p < add_parts ? add[part p] : 0),   p = 0, 1
// src: [l][N] per item, src_stride apart; add / out: [2][l][N] per item.  temp1: [l][rc][N], temp2: [2][rc][N]
// per item, both `per` apart.  out may alias add.
static hipError_t ckks_keyswitch_core(const Context& c, const u64* src, u64 src_stride, const u64* add, u64 add_stride,
                                      int add_parts, u64* outp, u64 out_stride, const u64* key, int depth, int batch,
                                      u64* temp1, u64* temp2, u64 per, hipStream_t st, unsigned phases,
                                      int galois_elt = 0)
{
    const int Q = c.Q_size, Qp = c.Qp_size;
    const int l = Q - depth, rc = Qp - depth;

    NttArgs a = c.ntt_args(0);
    // INTT(src), batch l per item (:919) -- out of place into the (not yet used)
    // accumulator region: src itself stays in the NTT domain because digit d
    // re-reduced into its own modulus d and transformed back is that limb
    a.in = src; a.out = temp2; a.mod_count = l; a.polys_per_item = l;
    a.in_item_stride = src_stride; a.out_item_stride = per;
    // digit decomposition src -> [l][rc][N] fused into the forward NTT's
    // first load; modulus order skips dropped primes                (:932-960)
    NttArgs dgt = c.ntt_args(0);
    dgt.in = temp2; dgt.out = temp1; dgt.mod_count = rc; dgt.polys_per_item = l * rc; dgt.decomp_mods = rc;
    dgt.in_item_stride = per; dgt.out_item_stride = per;
    dgt.mod_order = c.tab.new_prime_locations + triangle_offset(Qp, depth);
    fill_int_slots(c, dgt, c.hv.new_prime_locations.data() + triangle_offset(Qp, depth));
    // When the decomposing column pass is the multi-modulus kernel (one launch for the whole batch), it also
    // finishes the inverse transform of its source tiles: only the row stages of the INTT run on their own.
    const bool fuse_inv = use_fused_row_mac(c, rc, batch) && c.fuse_inverse && (long) l * rc * batch <= 65535 &&
                          ntt_decomp_uses_multi(dgt, l * rc * batch);
    if (phases & RELIN_PHASE_INTT_C2) {
        if (fuse_inv) TRY(ntt_launch_inv_rows(a, l * batch, st));
        else TRY(ntt_launch(a, l * batch, true, st));
    }
    dgt.src_inv = fuse_inv ? 1 : 0;
    dgt.single_decomp_ok = 1; // temp2 -> temp1, no epilogue
    a = dgt;
    // forward NTT of the digits + inner product with the key      (:956-988)
    const int which = ((phases & RELIN_PHASE_COLUMN) ? 1 : 0) | ((phases & RELIN_PHASE_ROW_MAC) ? 2 : 0);
    // Mod-down inside the fused kernels: the inner product of the P slot first, its INTT, the mod-down's column pass
    // (T, the P limb at every q_j, into the Q slots of temp2, which are never written as accumulators), and only then
    // the inner product of the Q slots, whose workgroups finish T's row stages and apply the mod-down to their sums
    // while they are still in registers: the 2 l accumulator limbs are neither stored nor read back, and the mod-down
    // row pass has no launch of its own.  ROW_MAC covers both inner-product launches.
    const bool in_mac = use_moddown_in_mac(c, key, l, rc, batch);
    if (which) // with in_mac: the P slot (slot l) only
        TRY(keyswitch_ntt_mac(c, a, key, temp2, per, l, rc, l, depth, src, src_stride, batch, st, which, in_mac ? l : 0,
                              in_mac ? 1 : 0));
    const NttArgs dgt_args = a;
    // INTT of the two P-limb polynomials only                        (:996)
    a = c.ntt_args(0);
    a.in = temp2; a.out = temp2; a.mod_count = 1; a.mod_offset = Q; a.polys_per_item = 2;
    a.in_item_stride = a.out_item_stride = per;
    a.poly_order = c.tab.new_input_locations + 2 * depth;
    // the same fusion for the mod-down transform, whose source is the inverse transform of the P limbs
    NttArgs md = c.ntt_args(0);
    md.in = temp2; md.out = temp1; md.mod_count = l; md.polys_per_item = 2 * l;
    md.in_item_stride = md.out_item_stride = per;
    md.decomp_mods = l; md.decomp_in_mul = l + 1; md.decomp_in_add = l;
    md.half_on = 1; md.half_src_mod = Q;
    fill_int_slots(c, md, nullptr);
    const bool fuse_inv_p = c.fused_moddown && c.fuse_inverse && (long) 2 * l * batch <= 65535 &&
                            ntt_decomp_uses_multi(md, 2 * l * batch);
    if (phases & RELIN_PHASE_INTT_P) {
        if (fuse_inv_p) TRY(ntt_launch_inv_rows(a, 2 * batch, st));
        else TRY(ntt_launch(a, 2 * batch, true, st));
    }
    if (in_mac) {
        if (phases & RELIN_PHASE_MODDOWN) {
            a = md;
            a.out = temp2; a.decomp_out_mul = l + 1; // T of part p, limb j: slot j of part p in temp2 [2][l+1][N]
            a.half = c.hv.half; a.half_mod = c.tab.half_mod;
            a.src_inv = fuse_inv_p ? 1 : 0;
            TRY(ntt_launch_fwd_col(a, 2 * l * batch, st));
        }
        if (!(phases & RELIN_PHASE_ROW_MAC)) return hipSuccess;
        KsMacArgs::Tail t{};
        t.on = 1;
        t.T = temp2; t.T_item_stride = per;
        t.ct = add; t.ct_item_stride = add_stride; t.ct_parts = add_parts;
        t.out = outp; t.out_item_stride = out_stride;
        t.inv = c.tab.last_q_modinv;
        t.limbs = l;
        t.galois_inv = galois_elt ? (unsigned) inv_mod_2n((u64) galois_elt, 2 * c.n) : 0u;
        return keyswitch_ntt_mac(c, dgt_args, key, temp2, per, l, rc, l, depth, src, src_stride, batch, st, 2, 0, l, &t);
    }
    if (!(phases & RELIN_PHASE_MODDOWN)) return hipSuccess;
    // stage one: P limb (+half) reduced into every q_j               (:1003)
    if (!c.fused_moddown)
        TRY(rns_moddown_stage_one(temp2, per, temp1, per, c.moddown(depth), batch, st));
    // forward NTT of that (:1011) with stage one as its load transform and stage two -- (x - last) * P^-1 + add, written to
    // out parts 0,1 (:1015) -- as the epilogue of its row pass
    a = c.ntt_args(0);
    a.in = temp1; a.out = temp1; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = a.out_item_stride = per;
    if (c.fused_moddown) {
        // input: the P limb (slot l) of each of the two parts of temp2 [2][l+1][N]
        a.in = temp2; a.decomp_mods = l; a.decomp_in_mul = l + 1; a.decomp_in_add = l;
        a.half_on = 1; a.half_src_mod = Q; a.half = c.hv.half; a.half_mod = c.tab.half_mod;
        a.epi.on = 1;
        a.epi.ks = temp2; a.epi.ks_item_stride = per; a.epi.ks_part_limbs = l + 1;
        a.epi.ct = add; a.epi.ct_item_stride = add_stride; a.epi.ct_parts = add_parts;
        a.epi.out = outp; a.epi.out_item_stride = out_stride;
        a.epi.inv = c.tab.last_q_modinv;
        a.epi.limbs = l;
        a.epi.galois_inv = galois_elt ? (unsigned) inv_mod_2n((u64) galois_elt, 2 * c.n) : 0u;
        a.src_inv = fuse_inv_p ? 1 : 0;
        a.single_decomp_ok = 1; // source: the P-limb slots of temp2; the epilogue reads its Q-limb slots and `add`, writes `outp`
        fill_int_slots(c, a, nullptr);
        return ntt_launch(a, 2 * l * batch, false, st);
    }
    if (add_parts != 2 || galois_elt) return hipErrorInvalidValue; // the stand-alone stage two adds both parts (relinearize only)
    TRY(ntt_launch(a, 2 * l * batch, false, st));
    return rns_moddown_stage_two(temp1, per, temp2, per, add, add_stride, outp, out_stride, c.moddown(depth), 1, batch, st);
}

// ------------------------------------------------------------------ method II (P_size > 1)
static hipError_t dtoq(const Context& c, int lvl, const u64* in, u64 in_stride, u64* out, u64 out_stride, int l,
                       int level, int batch, hipStream_t st)
{
    const Context::M2Level& L = c.m2_levels[lvl];
    return rns_base_conversion_DtoQtilde(in, in_stride, out, out_stride, c.plan_qp.mods,
                                         c.tab.m2_matrix_mg + L.off_matrix, c.tab.m2_Mi_inv + L.off_mi,
                                         c.tab.m2_negprod_mg + L.off_prod, c.tab.m2_I_j + L.off_digits,
                                         c.tab.m2_I_location + L.off_digits, c.n_power, L.d, L.rc, l, level,
                                         c.m2_width, batch, st);
}

// reference ckks/operator.cu:1025-1154
// CKKS key switching with several special primes, tail: acc [2][rc][N] (NTT domain) -> out [2][l][N] =
// moddown(acc) + ct (parts below add_parts; 0 = both) [-> Galois automorphism].  The reference runs the INTT of all
// 2 rc limbs, divide_round_lastq_extended_leveled_kernel, the NTT of 2 l limbs and an addition
// (ckks/operator.cu:1131-1149).  Here only the 2 P special limbs are inverse-transformed; from them one kernel
// forms, per limb of Q, the value u whose transform the forward pass's epilogue subtracts from the accumulated limb
// before multiplying by W0 = prod P_i^-1 (context.cpp m2_md_*): the same exact integer function, so the same
// residues.  scratch: [2][l][N] per item (`per` apart).
static hipError_t ckks_moddown_multi(const Context& c, u64* acc, u64* scratch, u64 per, const u64* ct, u64 cs,
                                     int add_parts, u64* out, u64 so, int depth, int galois_elt, int batch,
                                     hipStream_t st)
{
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size, P = c.P_size;
    const int l = Q - depth, rc = Qp - depth;
    for (int part = 0; part < 2; part++) {
        NttArgs a = c.ntt_args(0);
        a.in = a.out = acc + (u64) (part * rc + l) * n;
        a.mod_count = P; a.mod_offset = Q; a.polys_per_item = P;
        a.in_item_stride = a.out_item_stride = per;
        TRY(ntt_launch(a, P * batch, true, st));
    }
    TRY(rns_moddown_multi_stage_one(acc, per, scratch, per, c.moddown(depth), c.tab.m2_md_G, c.tab.m2_md_C, batch, st));
    NttArgs a = c.ntt_args(0);
    a.in = a.out = scratch; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = a.out_item_stride = per;
    a.epi.on = 1;
    a.epi.ks = acc; a.epi.ks_item_stride = per; a.epi.ks_part_limbs = rc;
    a.epi.ct = ct; a.epi.ct_item_stride = cs; a.epi.ct_parts = add_parts;
    a.epi.out = out; a.epi.out_item_stride = so;
    a.epi.inv = c.tab.m2_md_W0;
    a.epi.limbs = l;
    a.epi.galois_inv = galois_elt ? (unsigned) inv_mod_2n((u64) galois_elt, 2 * c.n) : 0u;
    return ntt_launch(a, 2 * l * batch, false, st);
}

// The reference-order tail of a CKKS rotation (ckks/operator.cu:1524-1541): INTT of the 2 rc accumulator limbs
// acc [2][rc][N], mod-down + Galois permutation with c0 of the coefficient-domain ciphertext coef [2][l][N] added (both
// `per` apart per item), NTT of the 2 l limbs of out.
static hipError_t ckks_rotate_tail(const Context& c, u64* acc, const u64* coef, u64 per, u64* out, u64 so, int galois_elt,
                                   int depth, int batch, hipStream_t st)
{
    const int Q = c.Q_size, Qp = c.Qp_size;
    const int l = Q - depth, rc = Qp - depth;
    NttArgs a = c.ntt_args(0);
    a.in = acc; a.out = acc; a.mod_count = rc; a.polys_per_item = 2 * rc;
    a.mod_order = c.tab.new_prime_locations + triangle_offset(Qp, depth);
    a.in_item_stride = a.out_item_stride = per;
    TRY(ntt_launch(a, 2 * rc * batch, true, st));                                          // :1524
    TRY(rns_moddown_permute(acc, per, coef, per, out, so, c.moddown(depth), galois_elt, batch, st)); // :1530
    a = c.ntt_args(0);
    a.in = out; a.out = out; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = a.out_item_stride = so;
    return ntt_launch(a, 2 * l * batch, false, st);                                        // :1541
}

// Key switch, method II, of part `add_parts` of each ciphertext with the parts below it added: c2 for relinearize
// (add_parts 2, out == ct; reference ckks/operator.cu:1025-1154), c1 for apply_galois (add_parts 1, then the
// automorphism galois_elt; :1561-1720).  Relinearize inverse-transforms c2 in place; a rotation inverse-transforms c1
// into a [2][l][N] coefficient-domain copy at the front of its workspace, and c0 too when its tail runs in the
// reference order.  Workspace: keyswitch_ws without (relinearize) or with the copy, one accumulator.
static hipError_t ckks_keyswitch_II(const Context& c, const u64* ct, u64 cs, int add_parts, u64* out, u64 so,
                                    const u64* key, int galois_elt, int depth, int batch, u64* ws, hipStream_t st)
{
    const int np = c.n_power;
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size;
    const int l = Q - depth, rc = Qp - depth;
    const int d = c.m2_levels[depth].d;
    const bool relin = add_parts == 2;
    // the mod-down as the epilogue of its forward transform (ckks_moddown_multi); a rotation's c0 then stays in the NTT
    // domain (see op_ckks_apply_galois)
    const bool ntt_domain = c.fused_moddown && (relin || c.ntt_galois);
    const KeySwitchWs w = keyswitch_ws(c, depth, !relin, 1);
    u64* coef = relin ? out : ws; // the coefficient-domain parts, coef_stride apart
    const u64 coef_stride = relin ? so : w.per;
    u64* digits = ws + w.digits; // [d][rc][N]
    u64* acc = ws + w.acc;       // [2][rc][N]
    const int first = (relin || ntt_domain) ? add_parts : 0; // first part inverse-transformed
    NttArgs a = c.ntt_args(0);
    a.in = ct + (u64) first * l * n; a.out = coef + (u64) first * l * n; a.mod_count = l;
    a.polys_per_item = (add_parts + 1 - first) * l;
    a.in_item_stride = cs; a.out_item_stride = coef_stride;
    TRY(ntt_launch(a, a.polys_per_item * batch, true, st));                                // :1052
    TRY(dtoq(c, depth, coef + (u64) add_parts * l * n, coef_stride, digits, w.per, l, depth, batch, st)); // :1065
    a = c.ntt_args(0);
    a.in = digits; a.out = digits; a.mod_count = rc; a.polys_per_item = d * rc;
    a.mod_order = c.tab.new_prime_locations + triangle_offset(Qp, depth);
    a.in_item_stride = a.out_item_stride = w.per;
    TRY(keyswitch_ntt_mac(c, a, key, acc, w.per, d, rc, l, depth, nullptr, 0, batch, st));  // :1095-1125
    // the front of the workspace (the digits of a relinearization, the coefficient-domain copy of a rotation) is free
    // again: scratch of the mod-down; ct_parts 0 adds both parts
    if (ntt_domain)
        return ckks_moddown_multi(c, acc, ws, w.per, ct, cs, relin ? 0 : add_parts, out, so, depth, galois_elt, batch, st);
    if (!relin) return ckks_rotate_tail(c, acc, ws, w.per, out, so, galois_elt, depth, batch, st);
    a.in = acc; a.out = acc; a.polys_per_item = 2 * rc;
    TRY(ntt_launch(a, 2 * rc * batch, true, st));                                          // :1131
    TRY(rns_moddown_extended(acc, w.per, nullptr, 0, ws, w.per, c.moddown(depth), 0, batch, st)); // :1136
    a = c.ntt_args(0);
    a.in = ws; a.out = ws; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = a.out_item_stride = w.per;
    TRY(ntt_launch(a, 2 * l * batch, false, st));                                          // :1145
    // addition(temp1, ct, ct): per-item strides differ, so one launch per item batch via copy-free add
    return rns_addition_strided(ws, w.per, ct, cs, out, so, c.plan_qp.mods, np, l, 2, batch, st); // :1149
}

// reference ckks/operator.cu:899-1023
hipError_t op_ckks_relinearize(const Context& c, u64* ct, u64 cs, const u64* key, int depth, int batch, u64* ws,
                               hipStream_t st, unsigned phases)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (c.P_size > 1) return ckks_keyswitch_II(c, ct, cs, 2, ct, cs, key, 0, depth, batch, ws, st);
    const int l = c.Q_size - depth;
    const KeySwitchWs w = keyswitch_ws(c, depth, false, 1);
    u64* temp1 = ws + w.digits; // [l][rc][N] per item, later [2][l][N]
    u64* temp2 = ws + w.acc;    // [2][rc][N] per item
    return ckks_keyswitch_core(c, ct + ((u64) l << (c.n_power + 1)), cs, ct, cs, 2, ct, cs, key, depth, batch, temp1,
                               temp2, w.per, st, phases);
}

// reference ckks/operator.cu:1156-1244
hipError_t op_ckks_rescale(const Context& c, u64* ct, u64 cs, int depth, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    const int np = c.n_power;
    const u64 n = c.n;
    const int Q = c.Q_size, P = c.P_size;
    const int l = Q - depth;
    const ModDown md = c.moddown(depth, true);
    const PairWs w = rescale_ws(c, depth);
    u64* temp1 = ws;            // [2][l-1][N]
    u64* temp2 = ws + w.second; // copy of ct, part stride l

    NttArgs a = c.ntt_args(0);
    a.in = ct; a.out = ct; a.mod_count = 1; a.mod_offset = l - 1; a.polys_per_item = 2;
    a.in_item_stride = a.out_item_stride = cs;
    a.poly_order = c.tab.new_input_locations + (depth + P) * 2;
    TRY(ntt_launch(a, 2 * batch, true, st));                                               // :1197
    if (c.fused_moddown) {
        // stage one (:1205) as the load transform and stage two (:1225) as the row-pass epilogue
        // of the forward NTT (:1214); the copy of the kept limbs (:1219) comes first because the
        // epilogue writes the compacted ciphertext over them
        a = c.ntt_args(0);
        a.in = ct; a.out = temp1; a.mod_count = l - 1; a.polys_per_item = 2 * (l - 1);
        a.in_item_stride = cs; a.out_item_stride = w.per;
        a.decomp_mods = l - 1; a.decomp_in_mul = l; a.decomp_in_add = l - 1;
        a.half_on = 1; a.half_src_mod = l - 1; a.half = c.hv.rescaled_half[depth];
        a.half_mod = md.half_mod;
        // The copy rides on the column pass when that is the per-polynomial kernel (one workgroup per kept limb
        // and tile: C2, 4.7 us of launch less); the multi-modulus kernel keeps its own launch for it.
        if (c.copy_along && !ntt_decomp_uses_multi(a, 2 * (l - 1) * batch)) {
            a.copy_src = ct; a.copy_src_item_stride = cs;
            a.copy_dst = temp2; a.copy_dst_item_stride = w.per;
            a.copy_part_limbs = l;
        } else {
            TRY(rns_copy_limbs(ct, (u64) l * n, cs, temp2, (u64) l * n, w.per, np, l - 1, 2, batch, st));
        }
        a.epi.on = 1;
        a.epi.ks = temp2; a.epi.ks_item_stride = w.per; a.epi.ks_part_limbs = l;
        a.epi.ct = nullptr; a.epi.ct_item_stride = 0;
        a.epi.out = ct; a.epi.out_item_stride = cs;
        a.epi.inv = md.last_q_modinv;
        a.epi.limbs = l - 1;
        return ntt_launch(a, 2 * (l - 1) * batch, false, st);
    }
    TRY(rns_moddown_stage_one(ct, cs, temp1, w.per, md, batch, st));                         // :1205
    a = c.ntt_args(0);
    a.in = temp1; a.out = temp1; a.mod_count = l - 1; a.polys_per_item = 2 * (l - 1);
    a.in_item_stride = a.out_item_stride = w.per;
    TRY(ntt_launch(a, 2 * (l - 1) * batch, false, st));                                    // :1214
    TRY(rns_copy_limbs(ct, (u64) l * n, cs, temp2, (u64) l * n, w.per, np, l - 1, 2, batch, st)); // :1219
    return rns_moddown_stage_two(temp1, w.per, temp2, w.per, nullptr, 0, ct, cs, md, 0, batch, st); // :1225
}

// reference ckks/operator.cu:3963-4033 without its key switches (mod_up_from_q0: INTT of the two q_0 limbs, mod_raise_kernel
// into [2][Q][N], NTT of all 2 Q limbs).  Here the lift is the load transform of the forward pass -- the mod-down's
// "(v + half) mod q_0 mod q_j - half mod q_j" with half = (q_0 + 1) / 2 (context.cpp mod_raise_half_mod), which is the
// residue of the centred representative -- and limb 0, whose transform would give the input back, is copied: no
// coefficient-domain [2][L][N] is written or read.  Every degree and launch size is served this way.
// k1 > 1 (the refresh's pre-multiplier, k1 < q_0): the raise of k1 * ct.  The copy of limb 0 becomes rns_scale_q0, which
// leaves k1 v mod q_0 in the workspace too; the inverse transform then runs there in place.  k1 == 1: the launches below
// are op_ckks_mod_raise's.
static hipError_t mod_raise_scaled(const Context& c, const u64* ct, u64 cs, u64 k1, u64* out, u64 so, int out_depth,
                                   int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    const u64 n = c.n, per = mod_raise_ws(c);
    const int L = c.Q_size - out_depth, t = L - 1; // limbs of the result, of them lifted
    if (k1 == 1) TRY(rns_copy_limbs(ct, n, cs, out, (u64) L * n, so, c.n_power, 1, 2, batch, st));
    else TRY(rns_scale_q0(ct, cs, k1, out, (u64) L * n, so, t < 1 ? nullptr : ws, per, c.plan_qp.mods, c.n_power, batch, st));
    if (t < 1) return hipSuccess;
    NttArgs inv = c.ntt_args(0);
    inv.in = k1 == 1 ? ct : ws; inv.out = ws; inv.mod_count = 1; inv.polys_per_item = 2;
    inv.in_item_stride = k1 == 1 ? cs : per; inv.out_item_stride = per;
    NttArgs a = c.ntt_args(0);
    a.in = ws; a.out = out + n; // digit p (part p), target slot k: limb 1 + k of part p
    a.mod_count = t; a.mod_offset = 1; a.polys_per_item = 2 * t;
    a.in_item_stride = per; a.out_item_stride = so;
    a.decomp_mods = t; a.decomp_out_mul = L;
    a.half_on = 1; a.half_src_mod = 0; a.half = c.hv.mod_raise_half; a.half_mod = c.tab.mod_raise_half_mod;
    a.single_decomp_ok = 1; // ws -> out
    fill_int_slots(c, a, nullptr);
    const bool fuse_inv = c.fuse_inverse && (long) 2 * t * batch <= 65535 && ntt_decomp_uses_multi(a, 2 * t * batch);
    if (fuse_inv) TRY(ntt_launch_inv_rows(inv, 2 * batch, st));
    else TRY(ntt_launch(inv, 2 * batch, true, st));
    a.src_inv = fuse_inv ? 1 : 0;
    return ntt_launch(a, 2 * t * batch, false, st);
}

hipError_t op_ckks_mod_raise(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, int out_depth, int batch, u64* ws,
                             hipStream_t st)
{
    return mod_raise_scaled(c, ct, cs, 1, out, so, out_depth, batch, ws, st);
}

// reference ckks/operator.cu:1422-1559
hipError_t op_ckks_apply_galois(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* key,
                                int galois_elt, int depth, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (c.P_size > 1) return ckks_keyswitch_II(c, ct, cs, 1, out, so, key, galois_elt, depth, batch, ws, st);
    const int np = c.n_power;
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size;
    const int l = Q - depth, rc = Qp - depth;
    const KeySwitchWs w = keyswitch_ws(c, depth, true, 1);
    u64* temp0 = ws;            // [2][l][N] coefficient-domain copy of ct
    u64* temp2 = ws + w.digits; // [l][rc][N]
    u64* temp3 = ws + w.acc;    // [2][rc][N]

    if (c.fused_moddown && c.ntt_galois) {
        // The key switch of c1 exactly as relinearize does it (c0 added to part 0 by the mod-down epilogue), all
        // in the NTT domain, and the automorphism last, as a slot gather of both parts.  Against the reference's
        // order (INTT of both parts, ..., INTT of 2 rc limbs, mod-down + permute in the coefficient domain, NTT
        // of 2 l limbs) this never transforms c0, inverse-transforms 2 instead of 2 rc accumulator limbs and has
        // no scattered stores; the residues are the same (the permutation commutes with the transform, the
        // mod-down is the same exact integer function either way).
        if (c.galois_scatter)
            return ckks_keyswitch_core(c, ct + (u64) l * n, cs, ct, cs, 1, out, so, key, depth, batch, temp2, temp3, w.per, st,
                                       RELIN_PHASE_ALL, galois_elt);
        TRY(ckks_keyswitch_core(c, ct + (u64) l * n, cs, ct, cs, 1, temp0, w.per, key, depth, batch, temp2, temp3, w.per, st,
                                RELIN_PHASE_ALL));
        return rns_permute_ntt(temp0, w.per, out, so, galois_elt, np, 2 * l, batch, st);
    }
    NttArgs a = c.ntt_args(0);
    a.in = ct; a.out = temp0; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = cs; a.out_item_stride = w.per;
    TRY(ntt_launch(a, 2 * l * batch, true, st));                                           // :1461
    a = c.ntt_args(0); // ckks_duplicate_kernel fused into the NTT load          :1467-1494
    a.in = temp0 + (u64) l * n; a.out = temp2; a.mod_count = rc; a.polys_per_item = l * rc; a.decomp_mods = rc;
    a.in_item_stride = a.out_item_stride = w.per;
    a.mod_order = c.tab.new_prime_locations + triangle_offset(Qp, depth);
    TRY(keyswitch_ntt_mac(c, a, key, temp3, w.per, l, rc, l, depth, ct + (u64) l * n, cs, batch, st)); // :1490-1520
    return ckks_rotate_tail(c, temp3, temp0, w.per, out, so, galois_elt, depth, batch, st);
}

// reference bfv/operator.cu:336-430
hipError_t op_bfv_multiply(const Context& c, const u64* ct1, u64 s1, const u64* ct2, u64 s2, u64* out, u64 so,
                           int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    const int np = c.n_power;
    const u64 n = c.n;
    const int L = c.Q_size + c.bsk_size;
    const PairWs w = bfv_multiply_ws(c);
    u64* temp1 = ws;            // [4][L][N]
    u64* temp2 = ws + w.second; // [3][L][N]
    TRY(rns_fast_convertion(ct1, s1, ct2, s2, temp1, w.per, c.behz, np, batch, st));         // :364
    NttArgs a = c.ntt_args(1);
    a.in = temp1; a.out = temp1; a.mod_count = L; a.polys_per_item = 4 * L;
    a.in_item_stride = a.out_item_stride = w.per;
    TRY(ntt_launch(a, 4 * L * batch, false, st));                                          // :393
    a.in = temp2; a.out = temp2; a.polys_per_item = 3 * L;
    if (c.fused_tensor) {
        // the tensor product (:399) as the load transform of the inverse transform (:410): [3][L][N] is never stored
        a.tensor_in = temp1; a.tensor_item_stride = w.per; a.tensor_limbs = L;
    } else {
        TRY(rns_cross_multiplication(temp1, w.per, temp1 + (u64) 2 * L * n, w.per, temp2, w.per, c.plan_merge.mods, np, L,
                                     batch, st));                                          // :399
    }
    TRY(ntt_launch(a, 3 * L * batch, true, st));                                           // :410
    return rns_fast_floor(temp2, w.per, out, so, c.behz, np, batch, st);                     // :416
}

// BFV key switching, tail: acc [2][Q'][N] (NTT domain, `per` apart) -> INTT -> divide by the special prime with
// rounding -> + ct (parts below add_parts) [-> Galois permutation] -> out [2][Q][N].  The reference runs the INTT
// of all 2 Q' limbs and then divide_round_lastq(_permute_bfv)_kernel (bfv/operator.cu:571-576, 846-853); here the
// two P limbs are inverse-transformed first and the division is the epilogue of the Q limbs' inverse transform
// (NttInvEpilogue): the coefficient-domain accumulator is never written or read back.
static hipError_t bfv_intt_moddown(const Context& c, u64* acc, u64 per, const u64* ct, u64 cs, int add_parts, u64* out,
                                   u64 so, int galois_elt, int batch, hipStream_t st)
{
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size;
    for (int part = 0; part < 2; part++) {
        NttArgs a = c.ntt_args(0);
        a.in = a.out = acc + (u64) (part * Qp + Q) * n;
        a.mod_count = 1; a.mod_offset = Q; a.polys_per_item = 1;
        a.in_item_stride = a.out_item_stride = per;
        TRY(ntt_launch(a, batch, true, st));
    }
    NttArgs a = c.ntt_args(0);
    a.in = a.out = acc; a.mod_count = Qp; a.polys_per_item = 2 * Qp;
    a.in_item_stride = a.out_item_stride = per;
    a.iepi.on = 1; a.iepi.limbs = Q; a.iepi.add_parts = add_parts; a.iepi.p_mod = Q; a.iepi.galois_elt = galois_elt;
    a.iepi.half = c.hv.half; a.iepi.half_mod = c.tab.half_mod; a.iepi.inv = c.tab.last_q_modinv;
    a.iepi.ct = ct; a.iepi.ct_item_stride = cs;
    a.iepi.out = out; a.iepi.out_item_stride = so;
    return ntt_launch(a, 2 * Qp * batch, true, st);
}

// BFV key switching with several special primes, tail: acc [2][Q'][N] (NTT domain) -> out [2][Q][N] = moddown(acc) + ct
// (parts below add_parts) [-> Galois permutation].  The reference inverse-transforms all 2 Q' limbs and runs
// divide_round_lastq_extended_kernel / divide_round_lastq_permute_bfv_kernel (bfv/operator.cu:657-667, 948-963).  Here
// the 2 P special limbs are inverse-transformed first, one kernel forms u = sum_i lh_i G_i - C per limb of Q from them
// (the chain among the special limbs run once per coefficient, context.cpp m2_md_*), and the division (x - u) * W0,
// the added ciphertext and the permutation are the epilogue of the Q limbs' inverse transform (NttInvEpilogue::u):
// the same exact integer function, the coefficient-domain accumulator is never written or read back.
// scratch: [2][Q][N] per item (`per` apart).
static hipError_t bfv_intt_moddown_multi(const Context& c, u64* acc, u64* scratch, u64 per, const u64* ct, u64 cs,
                                         int add_parts, u64* out, u64 so, int galois_elt, int batch, hipStream_t st)
{
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size, P = c.P_size;
    for (int part = 0; part < 2; part++) {
        NttArgs a = c.ntt_args(0);
        a.in = a.out = acc + (u64) (part * Qp + Q) * n;
        a.mod_count = P; a.mod_offset = Q; a.polys_per_item = P;
        a.in_item_stride = a.out_item_stride = per;
        TRY(ntt_launch(a, P * batch, true, st));
    }
    TRY(rns_moddown_multi_stage_one(acc, per, scratch, per, c.moddown(0), c.tab.m2_md_G, c.tab.m2_md_C, batch, st));
    NttArgs a = c.ntt_args(0);
    a.in = a.out = acc; a.mod_count = Qp; a.polys_per_item = 2 * Qp;
    a.in_item_stride = a.out_item_stride = per;
    a.iepi.on = 1; a.iepi.limbs = Q; a.iepi.p_count = P; a.iepi.add_parts = add_parts; a.iepi.p_mod = Q;
    a.iepi.galois_elt = galois_elt;
    a.iepi.inv = c.tab.m2_md_W0;
    a.iepi.u = scratch; a.iepi.u_item_stride = per;
    a.iepi.ct = ct; a.iepi.ct_item_stride = cs;
    a.iepi.out = out; a.iepi.out_item_stride = so;
    return ntt_launch(a, 2 * Qp * batch, true, st);
}

// BFV key switch of part `add_parts` of each ciphertext with the parts below it added: c2 for relinearize (add_parts 2,
// out == ct; reference bfv/operator.cu:505-583, 585-672), c1 for apply_galois (add_parts 1, then the Galois permutation
// galois_elt; :771-864, 866-973).  c0 is read straight from ct instead of being copied aside: a rotation's out must not
// alias ct.  Method I decomposes into digits in the forward NTT's load (cipher_broadcast_kernel / bfv_duplicate_kernel),
// method II converts them first (base_conversion_DtoQtilde).
static hipError_t bfv_keyswitch(const Context& c, const u64* ct, u64 cs, int add_parts, u64* out, u64 so,
                                const u64* key, int galois_elt, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size;
    const bool m2 = c.P_size > 1;
    const int digits = m2 ? c.m2_levels[0].d : Q;
    const KeySwitchWs w = keyswitch_ws(c, 0, false, 1);
    u64* temp1 = ws + w.digits; // [digits][Q'][N]
    u64* temp2 = ws + w.acc;    // [2][Q'][N]
    const u64* src = ct + (u64) add_parts * Q * n;
    NttArgs a = c.ntt_args(0);
    a.out = temp1; a.mod_count = Qp; a.polys_per_item = digits * Qp; a.out_item_stride = w.per;
    if (m2) {
        TRY(dtoq(c, 0, src, cs, temp1, w.per, Q, 0, batch, st));
        a.in = temp1; a.in_item_stride = w.per;
    } else {
        a.in = src; a.in_item_stride = cs; a.decomp_mods = Qp;
    }
    TRY(keyswitch_ntt_mac(c, a, key, temp2, w.per, digits, Qp, Qp, 0, nullptr, 0, batch, st));
    if (c.fused_moddown) { // temp1 (the digits) is free again: scratch of the multi-prime mod-down
        if (m2) return bfv_intt_moddown_multi(c, temp2, temp1, w.per, ct, cs, add_parts, out, so, galois_elt, batch, st);
        return bfv_intt_moddown(c, temp2, w.per, ct, cs, add_parts, out, so, galois_elt, batch, st);
    }
    a = c.ntt_args(0);
    a.in = temp2; a.out = temp2; a.mod_count = Qp; a.polys_per_item = 2 * Qp;
    a.in_item_stride = a.out_item_stride = w.per;
    TRY(ntt_launch(a, 2 * Qp * batch, true, st));
    if (add_parts == 1)
        return rns_moddown_permute(temp2, w.per, ct, cs, out, so, c.moddown(0), galois_elt, batch, st);
    if (m2) return rns_moddown_extended(temp2, w.per, ct, cs, out, so, c.moddown(0), 1, batch, st);
    return rns_divide_round_lastq(temp2, w.per, ct, cs, out, so, c.moddown(0), 0, batch, st);
}

hipError_t op_bfv_relinearize(const Context& c, u64* ct, u64 cs, const u64* key, int batch, u64* ws, hipStream_t st)
{
    return bfv_keyswitch(c, ct, cs, 2, ct, cs, key, 0, batch, ws, st);
}

hipError_t op_bfv_apply_galois(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* key,
                               int galois_elt, int batch, u64* ws, hipStream_t st)
{
    return bfv_keyswitch(c, ct, cs, 1, out, so, key, galois_elt, batch, ws, st);
}

// Hoisted rotations: fast_single_hoisting_rotation_ckks_method_I / _II (reference ckks/operator.cu:4674-4953,
// 5092-5446).  The reference computes, for every requested Galois element, the same INTT of the ciphertext, the
// same digit decomposition (method I: ckks_duplicate_kernel, method II: base_conversion_DtoQtilde) and the same
// forward NTT of the digits -- none of them depends on the element -- and then the key inner product, the INTT,
// the mod-down + permutation and the final NTT that do.  Here the shared part runs once: the coefficient-domain
// ciphertext and the NTT-domain digits stay in the workspace while the per-element part walks the keys, so every
// output is bit-identical to the reference's (and to `count` separate hegpu_ckks_apply_galois calls).
// out: [count][2][l][N] per ciphertext (`so` apart), entry i at i * 2 l N; galois_elts[i] == 0 copies the input
// (global_memory_replace_kernel, :4708 / :5141).  Workspace: keyswitch_ws with the copy and `group` accumulators, that is
// OP_CKKS_GALOIS for group 1 and OP_CKKS_ROTATE_HOISTED for group 4 (ops_rotate_hoisted_accumulators tells which fits).
hipError_t op_ckks_rotate_hoisted(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* const* keys,
                                  const int* galois_elts, int count, int depth, int batch, u64* ws, hipStream_t st,
                                  int group)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    const int np = c.n_power;
    const u64 n = c.n;
    const int Q = c.Q_size, Qp = c.Qp_size;
    const int l = Q - depth, rc = Qp - depth;
    const bool m2 = c.P_size > 1;
    const int digits = m2 ? c.m2_levels[depth].d : l;
    if (group != 1 && group != 4) return hipErrorInvalidValue;
    if (digits > 16) group = 1; // rns_keyswitch_mac_keys keeps the digits of a coefficient in 16 registers
    const KeySwitchWs w = keyswitch_ws(c, depth, true, group);
    u64* temp0 = ws;            // [2][l][N] coefficient-domain copy of ct
    u64* temp2 = ws + w.digits; // [digits][rc][N] NTT-domain digits
    u64* temp3 = ws + w.acc;    // [group][2][rc][N]
    const Mod* mods = c.plan_qp.mods;
    const int* order = c.tab.new_prime_locations + triangle_offset(Qp, depth);
    const u64 ct_words = (u64) 2 * l * n;
    bool any = false;
    for (int i = 0; i < count; i++) {
        if (galois_elts[i] == 0)
            TRY(rns_copy_limbs(ct, (u64) l * n, cs, out + (u64) i * ct_words, (u64) l * n, so, np, l, 2, batch, st));
        else if (!keys[i]) return hipErrorInvalidValue;
        else any = true;
    }
    if (!any) return hipSuccess;
    {   // a single element has nothing to share: the fused key-switch path of the plain operator is faster
        int nz = 0, which = -1;
        for (int i = 0; i < count; i++)
            if (galois_elts[i] != 0) { nz++; which = i; }
        if (nz == 1)
            return op_ckks_apply_galois(c, ct, cs, out + (u64) which * ct_words, so, keys[which], galois_elts[which], depth,
                                        batch, ws, st);
    }

    // With the mod-down fused into its transform every element stays in the NTT domain -- inner product, INTT of
    // the special limbs, mod-down transform whose epilogue adds c0 and scatters through the automorphism (see
    // op_ckks_apply_galois / ckks_moddown_multi).  c0 is never transformed, so only c1 goes through the shared INTT.
    const bool ntt_domain = c.fused_moddown && c.ntt_galois;
    // ---- shared: INTT of both parts (of c1 only: ntt_domain), digits, forward NTT of the digits
    NttArgs a = c.ntt_args(0);
    a.in = ct; a.out = temp0; a.mod_count = l; a.polys_per_item = 2 * l;
    a.in_item_stride = cs; a.out_item_stride = w.per;
    if (ntt_domain) {
        a.in = ct + (u64) l * n; a.out = temp0 + (u64) l * n; a.polys_per_item = l;
        TRY(ntt_launch(a, l * batch, true, st));
    } else {
        TRY(ntt_launch(a, 2 * l * batch, true, st));
    }
    a = c.ntt_args(0);
    a.out = temp2; a.mod_count = rc; a.polys_per_item = digits * rc; a.mod_order = order;
    a.in_item_stride = a.out_item_stride = w.per;
    if (m2) {
        TRY(dtoq(c, depth, temp0 + (u64) l * n, w.per, temp2, w.per, l, depth, batch, st));
        a.in = temp2;
    } else {
        // digit d at modulus d is the NTT-domain limb of c1 itself
        a.in = temp0 + (u64) l * n; a.decomp_mods = rc; a.skip_identity = 1;
        TRY(rns_copy_diag(ct + (u64) l * n, cs, temp2, w.per, np, l, rc, batch, st));
    }
    TRY(ntt_launch(a, digits * rc * batch, false, st));

    // ---- per Galois element; with room for four accumulators the inner products of four elements share one read
    // of the digits (rns_keyswitch_mac_keys)
    int pending[4], npend = 0, next = 0;
    for (int i = 0; i < count; i++) {
        if (galois_elts[i] == 0) continue;
        u64* oi = out + (u64) i * ct_words;
        u64* acc = temp3;
        if (group > 1) {
            if (npend == next) { // start a new group
                npend = next = 0;
                const u64* gk[4];
                for (int j = i; j < count && npend < group; j++)
                    if (galois_elts[j] != 0) { pending[npend] = j; gk[npend++] = keys[j]; }
                TRY(rns_keyswitch_mac_keys(temp2, w.per, gk, npend, temp3, w.per, w.acc_words, mods, np, digits, rc, Qp, l, depth,
                                           batch, st));
            }
            acc = temp3 + (u64) next * w.acc_words; // pending[next] == i
            next++;
        } else {
            TRY(rns_keyswitch_mac(temp2, w.per, keys[i], temp3, w.per, mods, np, digits, rc, Qp, l, depth, batch, st));
        }
        if (ntt_domain) {
            // temp0 is free once the digits exist: scratch of the mod-down transform
            if (m2) TRY(ckks_moddown_multi(c, acc, temp0, w.per, ct, cs, 1, oi, so, depth, galois_elts[i], batch, st));
            else
                TRY(ckks_keyswitch_core(c, nullptr, 0, ct, cs, 1, oi, so, nullptr, depth, batch, temp0, acc, w.per, st,
                                        RELIN_PHASE_INTT_P | RELIN_PHASE_MODDOWN, galois_elts[i]));
            continue;
        }
        if (group > 1) return hipErrorInvalidValue; // the reference-order tail works on one accumulator
        TRY(ckks_rotate_tail(c, temp3, temp0, w.per, oi, so, galois_elts[i], depth, batch, st));
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ plaintext matrix x encrypted vector
// Workspace, per batch: A = max(n1, n2) ciphertexts (the baby rotations; once the inner sums exist, the rotated inner
// sums), B = n2 ciphertexts (the inner sums), then the key-switch workspace of the hoisted rotations with four
// accumulators (which is also enough for every apply_galois).
struct LinearTransformWs { u64 a_stride, b_stride, B, ks, total; };
static LinearTransformWs linear_transform_ws(const Context& c, int n1, int n2, int depth, int batch)
{
    const u64 ct_words = (u64) 2 * (c.Q_size - depth) * c.n;
    const u64 a_stride = (u64) (n1 > n2 ? n1 : n2) * ct_words, b_stride = (u64) n2 * ct_words;
    const u64 B = a_stride * batch, ks = B + b_stride * batch;
    return {a_stride, b_stride, B, ks, ks + ops_workspace_elems(c, OP_CKKS_ROTATE_HOISTED, depth, batch)};
}
size_t ops_linear_transform_workspace_elems(const Context& c, int n1, int n2, int depth, int batch)
{
    return linear_transform_ws(c, n1, n2, depth, batch).total;
}

// ---- chained giant steps: giant_parent makes a forest of the n2 terms, giant_elts[j] / giant_keys[j] are term j's link
// to its parent (a root's: to the result).  ops_giant_chain_check: nullptr, or what is wrong with the table.
static bool giant_chain_given(const int* giant_parent, int n2)
{
    if (!giant_parent) return false;
    for (int j = 0; j < n2; j++)
        if (giant_parent[j] != -1) return true;
    return false;
}

// the links to the root above term j, -1 if the walk does not end within n2 steps (a term that is its own ancestor)
static int giant_chain_depth(const int* giant_parent, int n2, int j)
{
    int d = 0;
    for (int at = giant_parent[j]; at != -1; at = giant_parent[at])
        if (++d >= n2) return -1;
    return d;
}

const char* ops_giant_chain_check(const int* giant_parent, int n2, const u64* const* giant_keys, const int* giant_elts)
{
    if (!giant_chain_given(giant_parent, n2)) return nullptr; // the direct mode: op_ckks_linear_transform's own checks
    for (int j = 0; j < n2; j++)
        if (giant_parent[j] < -1 || giant_parent[j] >= n2) return "a giant-step parent outside [-1, n2)";
    for (int j = 0; j < n2; j++)
        if (giant_chain_depth(giant_parent, n2, j) < 0) return "a giant step is its own ancestor";
    for (int j = 0; j < n2; j++)
        if (giant_elts[j] != 0 && !giant_keys[j]) return "Galois key not present!";
    return nullptr;
}

// S_j = inner_j + sum over the children k of j of galois(giant_elts[k], S_k); out = sum over the roots r of
// galois(giant_elts[r], S_r).  Deepest terms first.  The 2 n2 ciphertext places of A and B hold at most one value per term
// (its inner sum, its folded sum or the rotation of that) and the target of the launch in flight, so a free place always
// exists: a fold never writes over one of its terms (rns_ckks_sum_terms' out is __restrict__), apply_galois never over its
// input.  A single root writes `out` itself.
static hipError_t giant_chain_fold(const Context& c, u64* A, u64 a_stride, u64* B, u64 b_stride, u64* out, u64 so,
                                   int n2, const u64* const* giant_keys, const int* giant_elts, const int* giant_parent,
                                   int depth, int batch, u64* ks, hipStream_t st)
{
    const int l = c.Q_size - depth;
    const u64 ct_words = (u64) 2 * l * c.n;
    const Mod* mods = c.plan_qp.mods;
    // places 0 .. n2 - 1: B, n2 .. 2 n2 - 1: A; place j holds inner sum j
    auto at = [&](int p) { return p < n2 ? B + (u64) p * ct_words : A + (u64) (p - n2) * ct_words; };
    auto stride = [&](int p) { return p < n2 ? b_stride : a_stride; };
    bool used[32] = {};
    auto take = [&]() {
        int p = 0;
        while (used[p]) p++; // n2 + 1 of 2 n2 places are in use at the most
        used[p] = true;
        return p;
    };
    int place[16], level[16], roots = 0, deepest = 0;
    for (int j = 0; j < n2; j++) {
        place[j] = j;
        used[j] = true;
        level[j] = giant_chain_depth(giant_parent, n2, j);
        if (level[j] < 0) return hipErrorInvalidValue;
        if (giant_elts[j] != 0 && !giant_keys[j]) return hipErrorInvalidValue;
        deepest = std::max(deepest, level[j]);
        roots += giant_parent[j] == -1;
    }
    const u64* terms[16];
    u64 strides[16];
    for (int d = deepest; d >= 0; d--)
        for (int j = 0; j < n2; j++) {
            if (level[j] != d) continue;
            const bool last = d == 0 && roots == 1; // the only root: what it writes last is the result
            // fold the children, which are rotated already
            int count = 0, spent[16];
            for (int k = 0; k < n2; k++)
                if (giant_parent[k] == j) spent[count++] = k;
            if (count) {
                terms[0] = at(place[j]);
                strides[0] = stride(place[j]);
                for (int i = 0; i < count; i++) {
                    terms[i + 1] = at(place[spent[i]]);
                    strides[i + 1] = stride(place[spent[i]]);
                }
                const bool to_out = last && giant_elts[j] == 0;
                const int p = to_out ? -1 : take();
                TRY(rns_ckks_sum_terms(terms, strides, count + 1, to_out ? out : at(p), to_out ? so : stride(p), mods, c.n_power,
                                       l, batch, st));
                used[place[j]] = false;
                for (int i = 0; i < count; i++) used[place[spent[i]]] = false;
                place[j] = p;
            }
            // the link to the parent (a root's: to the result)
            if (giant_elts[j] != 0) {
                const int p = last ? -1 : take();
                TRY(op_ckks_apply_galois(c, at(place[j]), stride(place[j]), last ? out : at(p), last ? so : stride(p),
                                         giant_keys[j], giant_elts[j], depth, batch, ks, st));
                used[place[j]] = false;
                place[j] = p;
            }
        }
    if (roots == 1) return hipSuccess;
    int count = 0;
    for (int j = 0; j < n2; j++)
        if (giant_parent[j] == -1) {
            terms[count] = at(place[j]);
            strides[count++] = stride(place[j]);
        }
    return rns_ckks_sum_terms(terms, strides, count, out, so, mods, c.n_power, l, batch, st);
}

hipError_t op_ckks_linear_transform(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const u64* diags,
                                    int n_diag, const int* index, int n1, int n2, const u64* const* baby_keys,
                                    const int* baby_elts, const u64* const* giant_keys, const int* giant_elts, int depth,
                                    int batch, u64* ws, hipStream_t st, const int* giant_parent)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (n1 < 1 || n1 > 16 || n2 < 1 || n2 > 16) return hipErrorInvalidValue;
    const bool chained = giant_chain_given(giant_parent, n2);
    if (chained && ops_giant_chain_check(giant_parent, n2, giant_keys, giant_elts)) return hipErrorInvalidValue;
    const int l = c.Q_size - depth;
    const u64 ct_words = (u64) 2 * l * c.n;
    const LinearTransformWs w = linear_transform_ws(c, n1, n2, depth, batch);
    u64* A = ws;
    u64* B = ws + w.B;
    u64* ks = ws + w.ks;
    const Mod* mods = c.plan_qp.mods;
    // 1. baby rotations (a single identity step reads the input itself)
    const u64* rot = ct;
    u64 rot_stride = cs;
    if (!(n1 == 1 && baby_elts[0] == 0)) {
        const int group = (c.fused_moddown && c.ntt_galois) ? 4 : 1;
        TRY(op_ckks_rotate_hoisted(c, ct, cs, A, w.a_stride, baby_keys, baby_elts, n1, depth, batch, ks, st, group));
        rot = A;
        rot_stride = w.a_stride;
    }
    // 2. all inner sums; a single giant step without a rotation is the result
    const bool direct = n2 == 1 && giant_elts[0] == 0;
    TRY(rns_ckks_diag_mac(rot, rot_stride, n1, diags, n_diag, index, n2, direct ? out : B, direct ? so : w.b_stride, mods,
                          c.n_power, l, batch, st));
    if (direct) return hipSuccess;
    if (chained) // (n2 >= 2: a term has a parent)
        return giant_chain_fold(c, A, w.a_stride, B, w.b_stride, out, so, n2, giant_keys, giant_elts, giant_parent, depth,
                                batch, ks, st);
    // 3. giant rotations into A (the baby rotations are spent; apply_galois forbids out == in)
    const u64* terms[16];
    u64 strides[16];
    for (int j = 0; j < n2; j++) {
        const u64* inner = B + (u64) j * ct_words;
        terms[j] = inner;
        strides[j] = w.b_stride;
        if (giant_elts[j] == 0) continue;
        if (!giant_keys[j]) return hipErrorInvalidValue;
        u64* rotated = n2 == 1 ? out : A + (u64) j * ct_words; // a single term is the result
        const u64 rs = n2 == 1 ? so : w.a_stride;
        TRY(op_ckks_apply_galois(c, inner, w.b_stride, rotated, rs, giant_keys[j], giant_elts[j], depth, batch, ks, st));
        terms[j] = rotated;
        strides[j] = rs;
    }
    if (n2 == 1) return hipSuccess;
    // 4. one read of every term, one write
    return rns_ckks_sum_terms(terms, strides, n2, out, so, mods, c.n_power, l, batch, st);
}

// ------------------------------------------------------------------ CoeffToSlot / SlotToCoeff
// Workspace, per batch: T0 and T1, one ciphertext of the start depth each (the chain alternates between them: a linear
// transform may not write over its input), then the largest workspace any step needs (the linear transforms'; it holds
// the hoisted-rotation workspace, which is enough for apply_galois and larger than the rescale's).
struct EncodingTransformWs { u64 t_stride, T1, step, total; };
static EncodingTransformWs encoding_transform_ws(const Context& c, const LinearFactor* f, int count, int depth, int batch)
{
    u64 step = ops_workspace_elems(c, OP_CKKS_ROTATE_HOISTED, depth, batch);
    for (int k = 0; k < count; k++) step = std::max(step, linear_transform_ws(c, f[k].n1, f[k].n2, depth, batch).total);
    const u64 t_stride = (u64) 2 * (c.Q_size - depth) * c.n, T1 = t_stride * batch;
    return {t_stride, T1, 2 * T1, 2 * T1 + step};
}
size_t ops_encoding_transform_workspace_elems(const Context& c, const LinearFactor* f, int count, int depth, int batch)
{
    return encoding_transform_ws(c, f, count, depth, batch).total;
}

// `count` x (linear transform, rescale) from cur at depth d0, alternating between the two buffers; the last product goes
// to `last` (stride last_stride) if given.  Returns where the result is.
static hipError_t encoding_transform_chain(const Context& c, const u64*& cur, u64& cur_stride, u64* T0, u64* T1,
                                           u64 t_stride, u64* last, u64 last_stride, const LinearFactor* f, int count,
                                           int d0, int batch, u64* step_ws, hipStream_t st)
{
    for (int k = 0; k < count; k++) {
        u64* dst = (cur == T0) ? T1 : T0;
        u64 ds = t_stride;
        if (last && k == count - 1) {
            dst = last;
            ds = last_stride;
        }
        TRY(op_ckks_linear_transform(c, cur, cur_stride, dst, ds, f[k].diags, f[k].n_diag, f[k].index, f[k].n1, f[k].n2,
                                     f[k].baby_keys, f[k].baby_elts, f[k].giant_keys, f[k].giant_elts, d0 + k, batch,
                                     step_ws, st, f[k].giant_parent));
        TRY(op_ckks_rescale(c, dst, ds, d0 + k, batch, step_ws, st));
        cur = dst;
        cur_stride = ds;
    }
    return hipSuccess;
}

hipError_t op_ckks_coeff_to_slot(const Context& c, const u64* ct, u64 cs, u64* out0, u64* out1, u64 so,
                                 const LinearFactor* f, int count, const u64* conj_key, int depth, int batch, u64* ws,
                                 hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (count < 1 || depth + count + 1 >= c.Q_size) return hipErrorInvalidValue;
    const EncodingTransformWs w = encoding_transform_ws(c, f, count, depth, batch);
    u64* T0 = ws;
    u64* T1 = ws + w.T1;
    u64* step_ws = ws + w.step;
    const u64* cur = ct;
    u64 cur_stride = cs;
    TRY(encoding_transform_chain(c, cur, cur_stride, T0, T1, w.t_stride, nullptr, 0, f, count, depth, batch, step_ws, st));
    const int d = depth + count;
    u64* conj = (cur == T0) ? T1 : T0;
    TRY(op_ckks_apply_galois(c, cur, cur_stride, conj, w.t_stride, conj_key, 2 * (int) c.n - 1, d, batch, step_ws, st));
    return rns_ckks_conj_split(cur, cur_stride, conj, w.t_stride, out0, out1, so, c.tab.psi_half, c.plan_qp.mods, c.n_power,
                               c.Q_size - d, c.Q_size - d - 1, batch, st);
}

hipError_t op_ckks_slot_to_coeff(const Context& c, const u64* c0, u64 s0, const u64* c1, u64 s1, u64* out, u64 so,
                                 const LinearFactor* f, int count, int depth, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (count < 1 || depth + count + 1 >= c.Q_size) return hipErrorInvalidValue;
    const EncodingTransformWs w = encoding_transform_ws(c, f, count, depth, batch);
    u64* T0 = ws;
    u64* T1 = ws + w.T1;
    u64* step_ws = ws + w.step;
    TRY(rns_ckks_conj_merge(c0, s0, c1, s1, T0, w.t_stride, c.tab.psi_half, c.plan_qp.mods, c.n_power, c.Q_size - depth,
                            c.Q_size - depth - 1, batch, st));
    const u64* cur = T0;
    u64 cur_stride = w.t_stride;
    return encoding_transform_chain(c, cur, cur_stride, T0, T1, w.t_stride, out, so, f, count, depth + 1, batch, step_ws, st);
}

// ------------------------------------------------------------------ polynomial evaluation
const char* ops_poly_eval_check(const Context& c, const host::PolyStep* plan, int n_steps, int depth)
{
    using namespace host;
    if (!plan || n_steps < 1) return "empty plan";
    if (n_steps > 4096) return "a plan of more than 4096 steps"; // degree 255, the largest the planner takes, has under 600
    if (depth < 0 || depth >= c.Q_size) return "invalid depth";
    const int top = c.Q_size - 1 - depth;
    // (a product without a tail is three parts wide in its register; one with a tail -- the double-angle step that ends an
    // EvalMod plan -- sits in the product region and its tail writes two parts)
    if (plan[n_steps - 1].kind == POLY_STEP_POWER && plan[n_steps - 1].c == POLY_TAIL_NONE)
        return "the last step is a leaf, a combination or a power with a tail";
    std::vector<int> level((size_t) n_steps + 1);
    std::vector<char> spent((size_t) n_steps + 1, 0); // rescaled in place by the COMBINE that consumed it
    level[0] = top;
    auto reg_ok = [&](int r, int dst) { return r >= 0 && r < dst && !spent[(size_t) r]; };
    for (int k = 0; k < n_steps; k++) {
        const PolyStep& s = plan[k];
        const int dst = k + 1;
        if (s.dst != dst) return "a step does not write the register of its position";
        if (s.level < 0 || s.level > top) return "a level outside the ciphertext's";
        // (the polynomial's last step; an EvalMod plan goes on from it, its register then has the sum's limbs: poly_reg_words)
        if (s.rescale_after && s.kind != POLY_STEP_COMBINE) return "only a COMBINE step rescales its result";
        if (s.kind == POLY_STEP_POWER) {
            if (!reg_ok(s.a, dst) || !reg_ok(s.b, dst)) return "a register number out of range";
            if (s.c != POLY_TAIL_NONE && s.c != POLY_TAIL_ONE && !reg_ok(s.c, dst)) return "a register number out of range";
            const int la = level[(size_t) s.a], lb = level[(size_t) s.b];
            if (s.mul_level < 1 || s.mul_level != (la < lb ? la : lb)) return "a product not at the lower of its operands' levels";
            if (s.level > s.mul_level - 1 || (s.c >= 0 && s.level > level[(size_t) s.c])) return "a power above its operands' levels";
            if (s.c < 0 && s.level != s.mul_level - 1) return "a power without a register tail leaves one level below its product";
            if (s.c == POLY_TAIL_ONE && !(s.tail_const > -3.4e38 && s.tail_const < 3.4e38)) return "a tail constant out of range";
        } else if (s.kind == POLY_STEP_LEAF) {
            if (s.n_terms < 0 || s.n_terms > POLY_LEAF_MAX) return "a leaf of more than 15 power terms";
            for (int i = 0; i < s.n_terms; i++) {
                if (!reg_ok(s.term_reg[i], dst)) return "a register number out of range";
                if (level[(size_t) s.term_reg[i]] < s.level) return "a leaf above the level of a term";
            }
        } else if (s.kind == POLY_STEP_COMBINE) {
            if (!reg_ok(s.a, dst) || !reg_ok(s.b, dst) || !reg_ok(s.c, dst)) return "a register number out of range";
            if (s.a == 0) return "the input cannot be rescaled in place";
            const int la = level[(size_t) s.a] - (s.rescale_first ? 1 : 0), lb = level[(size_t) s.b];
            if (la < 0) return "no modulus left to rescale by";
            if (s.mul_level < 0 || s.mul_level != (la < lb ? la : lb)) return "a product not at the lower of its operands' levels";
            const int lr = level[(size_t) s.c];
            const int sum = s.level + (s.rescale_after ? 1 : 0);
            if (sum != (s.mul_level < lr ? s.mul_level : lr)) return "a sum not at the lower of its operands' levels";
            if (s.rescale_first && (s.a == s.b || s.a == s.c)) return "a register rescaled in place is read once";
            if (s.rescale_first) spent[(size_t) s.a] = 1;
        } else {
            return "unknown step kind";
        }
        level[(size_t) dst] = s.level;
    }
    return nullptr;
}

// words of register k + 1 per item
static u64 poly_reg_words(const Context& c, const host::PolyStep& s)
{
    const bool product_in_place = s.kind == host::POLY_STEP_POWER && s.c == host::POLY_TAIL_NONE;
    return (product_in_place ? (u64) 3 * (s.mul_level + 1) : (u64) 2 * (s.level + 1 + (s.rescale_after ? 1 : 0))) * c.n;
}

// The registers of every step but the last (which writes `out`), each a block of `batch` items; T: one three-part product
// per item; D: one operand copied down to a product's level; ks: the larger of the relinearize and rescale workspaces
struct PolyEvalWs { u64 t_stride, d_stride, T, D, ks, total; };
struct PolyReg { u64* p; u64 stride; int limbs; };
// reg (with ws): reg[k + 1] becomes the register step k writes
static PolyEvalWs poly_eval_ws(const Context& c, const host::PolyStep* plan, int n_steps, int depth, int batch,
                               u64* ws = nullptr, PolyReg* reg = nullptr)
{
    u64 at = 0;
    for (int k = 0; k + 1 < n_steps; k++) {
        const u64 words = poly_reg_words(c, plan[k]);
        if (reg) reg[k + 1] = {ws + at, words, plan[k].level + 1};
        at += words * batch;
    }
    const u64 t_stride = (u64) 3 * (c.Q_size - depth) * c.n, d_stride = (u64) 2 * (c.Q_size - depth) * c.n;
    const u64 D = at + t_stride * batch, ks = D + d_stride * batch;
    return {t_stride, d_stride, at, D, ks, ks + std::max(ops_workspace_elems(c, OP_CKKS_RELIN, depth, batch),
                                                         ops_workspace_elems(c, OP_CKKS_RESCALE, depth, batch))};
}
size_t ops_poly_eval_workspace_elems(const Context& c, const host::PolyStep* plan, int n_steps, int depth, int batch)
{
    return poly_eval_ws(c, plan, n_steps, depth, batch).total;
}

hipError_t op_ckks_poly_eval(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const host::PolyStep* plan,
                             int n_steps, const u64* relin_key, int depth, int batch, u64* ws, hipStream_t st)
{
    using namespace host;
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (ops_poly_eval_check(c, plan, n_steps, depth)) return hipErrorInvalidValue;
    const int np = c.n_power, Q = c.Q_size;
    const u64 n = c.n;
    const Mod* mods = c.plan_qp.mods;
    using Reg = PolyReg;
    std::vector<Reg> reg((size_t) n_steps + 1);
    reg[0] = {const_cast<u64*>(ct), cs, Q - depth}; // never written: ops_poly_eval_check keeps register 0 out of every dst
    const PolyEvalWs w = poly_eval_ws(c, plan, n_steps, depth, batch, ws, reg.data());
    reg[(size_t) n_steps] = {out, so, plan[n_steps - 1].level + 1};
    u64* T = ws + w.T;   // one three-part product per item
    u64* D = ws + w.D;   // one operand copied down to the product's level
    u64* ks = ws + w.ks; // relinearize / rescale workspace

    // reg[x] * reg[y] at level ml, relinearized, into dst ([3][ml + 1][N] per item, two parts on return)
    auto product = [&](const Reg& x, const Reg& y, int ml, u64* dst, u64 dst_stride) -> hipError_t {
        const int l = ml + 1;
        Reg in[2] = {x, y};
        for (Reg& r : in)
            if (r.limbs != l) { // at most one of the two sits above the product's level
                TRY(rns_copy_limbs(r.p, (u64) r.limbs * n, r.stride, D, (u64) l * n, w.d_stride, np, l, 2, batch, st));
                r = {D, w.d_stride, l};
            }
        TRY(op_ckks_multiply(c, in[0].p, in[0].stride, in[1].p, in[1].stride, dst, dst_stride, Q - l, batch, st));
        return op_ckks_relinearize(c, dst, dst_stride, relin_key, Q - l, batch, ks, st);
    };

    for (int k = 0; k < n_steps; k++) {
        const PolyStep& s = plan[k];
        const Reg& dst = reg[(size_t) k + 1];
        if (s.kind == POLY_STEP_POWER) {
            const bool in_place = s.c == POLY_TAIL_NONE;
            u64* prod = in_place ? dst.p : T;
            const u64 ps = in_place ? dst.stride : w.t_stride;
            TRY(product(reg[(size_t) s.a], reg[(size_t) s.b], s.mul_level, prod, ps));
            TRY(op_ckks_rescale(c, prod, ps, Q - (s.mul_level + 1), batch, ks, st));
            if (in_place) continue;
            const Reg* b = s.c >= 0 ? &reg[(size_t) s.c] : nullptr;
            TRY(rns_ckks_double_sub(prod, ps, s.mul_level, b ? b->p : nullptr, b ? b->stride : 0, b ? b->limbs : 0,
                                    s.tail_const, dst.p, dst.stride, mods, np, dst.limbs, batch, st));
        } else if (s.kind == POLY_STEP_LEAF) {
            const u64* terms[POLY_LEAF_MAX];
            u64 strides[POLY_LEAF_MAX];
            int limbs[POLY_LEAF_MAX];
            for (int i = 0; i < s.n_terms; i++) {
                const Reg& r = reg[(size_t) s.term_reg[i]];
                terms[i] = r.p;
                strides[i] = r.stride;
                limbs[i] = r.limbs;
            }
            TRY(rns_ckks_weighted_sum(terms, strides, limbs, &s.w[0][0], s.n_terms, s.w0[0], s.w0[1], dst.p, dst.stride,
                                      c.tab.psi_half, mods, np, dst.limbs, batch, st));
        } else {
            Reg q = reg[(size_t) s.a];
            if (s.rescale_first) {
                TRY(op_ckks_rescale(c, q.p, q.stride, Q - q.limbs, batch, ks, st));
                q.limbs -= 1;
            }
            TRY(product(q, reg[(size_t) s.b], s.mul_level, T, w.t_stride));
            const int sum_limbs = dst.limbs + (s.rescale_after ? 1 : 0);
            Reg terms2[2] = {{T, w.t_stride, s.mul_level + 1}, reg[(size_t) s.c]};
            for (Reg& r : terms2)
                if (r.limbs != sum_limbs) { // the product is relinearized: D is free again
                    TRY(rns_copy_limbs(r.p, (u64) r.limbs * n, r.stride, D, (u64) sum_limbs * n, w.d_stride, np, sum_limbs, 2, batch, st));
                    r = {D, w.d_stride, sum_limbs};
                }
            const u64* tp[2] = {terms2[0].p, terms2[1].p};
            const u64 tsd[2] = {terms2[0].stride, terms2[1].stride};
            TRY(rns_ckks_sum_terms(tp, tsd, 2, dst.p, dst.stride, mods, np, sum_limbs, batch, st));
            if (s.rescale_after) TRY(op_ckks_rescale(c, dst.p, dst.stride, Q - sum_limbs, batch, ks, st));
        }
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ the CKKS refresh
// Head (OP_CKKS_BOOTSTRAP, the part no plan or factor changes): per item k1 * ct [2][N], its dense -> sparse switch [2][N],
// the raise's coefficient-domain pair [2][N].  Then the raised ciphertext [2][cts_level + 1][N] per item, with switch keys
// a second one (a key switch does not write over its input), the two halves after CoeffToSlot as 2 * batch items
// [2][eval_level + 1][N], EvalMod's result as 2 * batch items, and the largest workspace of the five sequences.
struct BootstrapWs { u64 scaled, sparse, raise_ws, R, r_stride, R2, H, h_stride, E, e_stride, step, total; };
static u64 bootstrap_head_ws(const Context& c) { return ops_workspace_elems(c, OP_CKKS_BOOTSTRAP, 0, 1); }
static BootstrapWs bootstrap_ws(const Context& c, const host::BootstrapPlan& p, const host::PolyStep* eval_mod, int n_steps,
                                const LinearFactor* cts, const LinearFactor* stc, bool switch_keys, int batch)
{
    const u64 n = c.n, B = (u64) batch;
    const int Q = c.Q_size;
    BootstrapWs w{};
    w.scaled = 0;
    w.sparse = 2 * n * B;
    w.raise_ws = 4 * n * B;
    w.R = bootstrap_head_ws(c) * B;
    w.r_stride = (u64) 2 * (p.cts_level + 1) * n;
    w.R2 = w.R + w.r_stride * B;
    w.H = w.R2 + (switch_keys ? w.r_stride * B : 0);
    w.h_stride = (u64) 2 * (p.eval_level + 1) * n;
    w.E = w.H + w.h_stride * 2 * B;
    const host::PolyStep& last = eval_mod[n_steps - 1];
    w.e_stride = (u64) 2 * (last.level + 1 + (last.rescale_after ? 1 : 0)) * n;
    w.step = w.E + w.e_stride * 2 * B;
    u64 step = std::max(ops_encoding_transform_workspace_elems(c, cts, p.cts_pieces, Q - 1 - p.cts_level, batch),
                        ops_encoding_transform_workspace_elems(c, stc, p.stc_pieces, Q - 1 - p.stc_level, batch));
    step = std::max<u64>(step, ops_poly_eval_workspace_elems(c, eval_mod, n_steps, Q - 1 - p.eval_level, 2 * batch));
    if (switch_keys)
        step = std::max<u64>(step, std::max(ops_workspace_elems(c, OP_CKKS_GALOIS, Q - 1, batch),
                                            ops_workspace_elems(c, OP_CKKS_GALOIS, Q - 1 - p.cts_level, batch)));
    w.total = w.step + step;
    return w;
}

const char* ops_bootstrap_check(const Context& c, const host::BootstrapPlan& p, const host::PolyStep* eval_mod, int n_steps)
{
    const int Q = c.Q_size;
    if (c.scheme != SCHEME_CKKS) return "context scheme mismatch";
    if (p.cts_pieces < 1 || p.cts_pieces > host::BOOTSTRAP_MAX_PIECES || p.stc_pieces < 1 ||
        p.stc_pieces > host::BOOTSTRAP_MAX_PIECES)
        return "a piece count outside [1, 5]";
    if (p.cts_level < 1 || p.cts_level >= Q) return "the raise goes to a level the context has";
    if (p.eval_level != p.cts_level - p.cts_pieces - 1 || p.eval_level < 1) return "EvalMod starts pieces + 1 levels below CoeffToSlot";
    if (p.k1 < 1 || p.k1 >= c.primes[0]) return "the pre-multiplier lies in [1, q_0)";
    if (const char* why = ops_poly_eval_check(c, eval_mod, n_steps, Q - 1 - p.eval_level)) return why;
    const host::PolyStep& last = eval_mod[n_steps - 1];
    if (last.level != p.stc_level || last.scale != p.eval_out_scale) return "the EvalMod plan is not the one of the bootstrap plan";
    if (p.out_level != p.stc_level - 1 - p.stc_pieces || p.out_level < 0) return "SlotToCoeff needs pieces + 1 levels and one limb left";
    return nullptr;
}

size_t ops_bootstrap_workspace_elems(const Context& c, const host::BootstrapPlan& p, const host::PolyStep* eval_mod,
                                     int n_steps, const LinearFactor* cts, const LinearFactor* stc, bool switch_keys, int batch)
{
    return bootstrap_ws(c, p, eval_mod, n_steps, cts, stc, switch_keys, batch).total;
}

// x k1 -> [key switch to the sparse secret at depth Q - 1] -> raise -> [key switch back] -> CoeffToSlot -> ONE EvalMod over
// the 2 * batch halves -> SlotToCoeff.  Every step is the existing sequence; the only launch of its own is rns_scale_q0,
// and that only for k1 > 1: without switch keys it takes the place of the raise's copy of limb 0.
hipError_t op_ckks_bootstrap(const Context& c, const u64* ct, u64 cs, u64* out, u64 so, const host::BootstrapPlan& p,
                             const host::PolyStep* eval_mod, int n_steps, const LinearFactor* cts, const LinearFactor* stc,
                             const u64* conj_key, const u64* relin_key, const u64* swk_dense_to_sparse,
                             const u64* swk_sparse_to_dense, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (ops_bootstrap_check(c, p, eval_mod, n_steps) || !swk_dense_to_sparse != !swk_sparse_to_dense) return hipErrorInvalidValue;
    const bool keys = swk_dense_to_sparse != nullptr;
    const BootstrapWs w = bootstrap_ws(c, p, eval_mod, n_steps, cts, stc, keys, batch);
    const int Q = c.Q_size, raise_depth = Q - 1 - p.cts_level;
    const u64 n = c.n;
    u64* step_ws = ws + w.step;
    u64* R = ws + w.R;
    const u64* raised = R;
    if (!keys) {
        TRY(mod_raise_scaled(c, ct, cs, p.k1, R, w.r_stride, raise_depth, batch, ws + w.raise_ws, st));
    } else {
        const u64* cur = ct;
        u64 cur_stride = cs;
        if (p.k1 != 1) {
            TRY(rns_scale_q0(ct, cs, p.k1, ws + w.scaled, n, 2 * n, nullptr, 0, c.plan_qp.mods, c.n_power, batch, st));
            cur = ws + w.scaled;
            cur_stride = 2 * n;
        }
        TRY(op_ckks_apply_galois(c, cur, cur_stride, ws + w.sparse, 2 * n, swk_dense_to_sparse, 1, Q - 1, batch, step_ws, st));
        TRY(op_ckks_mod_raise(c, ws + w.sparse, 2 * n, R, w.r_stride, raise_depth, batch, ws + w.raise_ws, st));
        TRY(op_ckks_apply_galois(c, R, w.r_stride, ws + w.R2, w.r_stride, swk_sparse_to_dense, 1, raise_depth, batch, step_ws, st));
        raised = ws + w.R2;
    }
    u64* H = ws + w.H; // items [0, batch): the first half of the coefficients, [batch, 2 batch): the second
    TRY(op_ckks_coeff_to_slot(c, raised, w.r_stride, H, H + w.h_stride * batch, w.h_stride, cts, p.cts_pieces, conj_key,
                              raise_depth, batch, step_ws, st));
    u64* E = ws + w.E;
    TRY(op_ckks_poly_eval(c, H, w.h_stride, E, w.e_stride, eval_mod, n_steps, relin_key, Q - 1 - p.eval_level, 2 * batch,
                          step_ws, st));
    return op_ckks_slot_to_coeff(c, E, w.e_stride, E + w.e_stride * batch, w.e_stride, out, so, stc, p.stc_pieces,
                                 Q - 1 - p.stc_level, batch, step_ws, st);
}

// ------------------------------------------------------------------ the slim family of refreshes
// Per batch: the raise's coefficient-domain pair [2][N], the raised ciphertext [2][cts_level + 1][N], the real parts
// [2][eval_level + 1][N], then one region the three sequences use in turn: the two alternating ciphertexts and the step
// workspace of an encoding transform (SlotToCoeff at the input's depth, CoeffToSlot at the raise's) or the polynomial
// evaluator's workspace.  The SlotToCoeff result stays in that region until the raise has read it.
struct SlimBootstrapWs { u64 raise_ws, R, r_stride, H, h_stride, step, total; };
static SlimBootstrapWs slim_bootstrap_ws(const Context& c, const host::SlimBootstrapPlan& p, const host::PolyStep* trig,
                                         int n_steps, const LinearFactor* cts, const LinearFactor* stc, int batch)
{
    const u64 n = c.n, B = (u64) batch;
    const int Q = c.Q_size;
    SlimBootstrapWs w{};
    w.raise_ws = 0;
    w.R = mod_raise_ws(c) * B;
    w.r_stride = (u64) 2 * (p.cts_level + 1) * n;
    w.H = w.R + w.r_stride * B;
    w.h_stride = (u64) 2 * (p.eval_level + 1) * n;
    w.step = w.H + w.h_stride * B;
    u64 step = std::max(ops_encoding_transform_workspace_elems(c, cts, p.cts_pieces, Q - 1 - p.cts_level, batch),
                        ops_encoding_transform_workspace_elems(c, stc, p.stc_pieces, Q - 1 - p.in_level, batch));
    step = std::max<u64>(step, ops_poly_eval_workspace_elems(c, trig, n_steps, Q - 1 - p.eval_level, batch));
    w.total = w.step + step;
    return w;
}

const char* ops_slim_bootstrap_check(const Context& c, const host::SlimBootstrapPlan& p, const host::PolyStep* trig, int n_steps)
{
    const int Q = c.Q_size;
    if (c.scheme != SCHEME_CKKS) return "context scheme mismatch";
    if (p.cts_pieces < 1 || p.cts_pieces > host::BOOTSTRAP_MAX_PIECES || p.stc_pieces < 1 ||
        p.stc_pieces > host::BOOTSTRAP_MAX_PIECES)
        return "a piece count outside [1, 5]";
    if (p.in_level != p.stc_pieces || p.in_level >= Q) return "SlotToCoeff starts at the level of its piece count";
    if (p.cts_level < 1 || p.cts_level >= Q) return "the raise goes to a level the context has";
    if (p.eval_level != p.cts_level - p.cts_pieces - 1 || p.eval_level < 1) return "the polynomial starts pieces + 1 levels below CoeffToSlot";
    if (const char* why = ops_poly_eval_check(c, trig, n_steps, Q - 1 - p.eval_level)) return why;
    const host::PolyStep& last = trig[n_steps - 1];
    if (last.level != p.out_level || last.scale != p.eval_out_scale) return "the polynomial plan is not the one of the bootstrap plan";
    return nullptr;
}

size_t ops_slim_bootstrap_workspace_elems(const Context& c, const host::SlimBootstrapPlan& p, const host::PolyStep* trig,
                                          int n_steps, const LinearFactor* cts, const LinearFactor* stc, int batch)
{
    return slim_bootstrap_ws(c, p, trig, n_steps, cts, stc, batch).total;
}

// [ct + ct2] -> SlotToCoeff down to q_0 -> raise -> CoeffToSlot, conjugate, real part -> ONE polynomial at batch B into out.
// Every step is the existing sequence; the only kernel of its own is rns_ckks_conj_real.
hipError_t op_ckks_slim_bootstrap(const Context& c, const u64* ct, u64 cs, const u64* ct2, u64 cs2, u64* out, u64 so,
                                  const host::SlimBootstrapPlan& p, const host::PolyStep* trig, int n_steps,
                                  const LinearFactor* cts, const LinearFactor* stc, const u64* conj_key, const u64* relin_key,
                                  int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    if (ops_slim_bootstrap_check(c, p, trig, n_steps)) return hipErrorInvalidValue;
    const SlimBootstrapWs w = slim_bootstrap_ws(c, p, trig, n_steps, cts, stc, batch);
    const int Q = c.Q_size, in_depth = Q - 1 - p.in_level, raise_depth = Q - 1 - p.cts_level;
    u64* region = ws + w.step;
    // 1. SlotToCoeff on the one input, P_stc levels, no merge
    const EncodingTransformWs ws_stc = encoding_transform_ws(c, stc, p.stc_pieces, in_depth, batch);
    const u64* cur = ct;
    u64 cur_stride = cs;
    if (ct2) { // a gate: the modular sum of its two inputs
        TRY(rns_addition_strided(ct, cs, ct2, cs2, region, ws_stc.t_stride, c.plan_qp.mods, c.n_power, Q - in_depth, 2, batch, st));
        cur = region;
        cur_stride = ws_stc.t_stride;
    }
    TRY(encoding_transform_chain(c, cur, cur_stride, region, region + ws_stc.T1, ws_stc.t_stride, nullptr, 0, stc,
                                 p.stc_pieces, in_depth, batch, region + ws_stc.step, st));
    // 2. the raise of its q_0 limbs ([2][1][N] per item after the last rescale)
    u64* R = ws + w.R;
    TRY(op_ckks_mod_raise(c, cur, cur_stride, R, w.r_stride, raise_depth, batch, ws + w.raise_ws, st));
    // 3. CoeffToSlot, the conjugate, and the real part alone
    const EncodingTransformWs ws_cts = encoding_transform_ws(c, cts, p.cts_pieces, raise_depth, batch);
    u64* T0 = region;
    u64* T1 = region + ws_cts.T1;
    cur = R;
    cur_stride = w.r_stride;
    TRY(encoding_transform_chain(c, cur, cur_stride, T0, T1, ws_cts.t_stride, nullptr, 0, cts, p.cts_pieces, raise_depth,
                                 batch, region + ws_cts.step, st));
    const int d = raise_depth + p.cts_pieces;
    u64* conj = (cur == T0) ? T1 : T0;
    TRY(op_ckks_apply_galois(c, cur, cur_stride, conj, ws_cts.t_stride, conj_key, 2 * (int) c.n - 1, d, batch,
                             region + ws_cts.step, st));
    u64* H = ws + w.H;
    TRY(rns_ckks_conj_real(cur, cur_stride, conj, ws_cts.t_stride, H, w.h_stride, c.plan_qp.mods, c.n_power, Q - d, Q - d - 1,
                           batch, st));
    // 4. one plan, batch items
    return op_ckks_poly_eval(c, H, w.h_stride, out, so, trig, n_steps, relin_key, Q - 1 - p.eval_level, batch, region, st);
}

// ------------------------------------------------------------------ logic gates
hipError_t op_ckks_logic_gate(const Context& c, int gate, const u64* a, u64 as, const u64* b, int b_kind, u64 bs,
                              const u64* relin_key, double scale_one, u64* out, u64 so, int depth, int batch, u64* ws,
                              hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    int k[3];
    if (!logic_gate_coefficients(gate, k)) return hipErrorInvalidValue;
    const int np = c.n_power, l = c.Q_size - depth;
    const Mod* mods = c.plan_qp.mods;
    const BfvPlainScale none{};
    if (gate == LOGIC_NOT)
        return rns_gate_combine(false, k[0], k[1], k[2], a, as, l, nullptr, GATE_B_NONE, 0, 0, nullptr, 0, 0, scale_one,
                                nullptr, none, out, so, mods, np, l, batch, st);
    if (l < 2 || (b_kind != GATE_B_CIPHER && b_kind != GATE_B_PLAIN)) return hipErrorInvalidValue;
    const GateWs w = gate_ws(c, false, depth, batch);
    u64* prod = ws;
    u64* ks = ws + w.ks;
    if (b_kind == GATE_B_CIPHER) {
        TRY(op_ckks_multiply(c, a, as, b, bs, prod, w.ps, depth, batch, st));
        TRY(op_ckks_relinearize(c, prod, w.ps, relin_key, depth, batch, ks, st));
    } else {
        for (int i = 0; i < batch; i++) // cipherplain_kernel takes one ciphertext
            TRY(kg_pk_u(a + as * i, b + bs * i, prod + w.ps * i, mods, np, l, st));
    }
    TRY(op_ckks_rescale(c, prod, w.ps, depth, batch, ks, st));
    return rns_gate_combine(false, k[0], k[1], k[2], a, as, l, b, b_kind, bs, l, prod, w.ps, l - 1, scale_one, nullptr, none,
                            out, so, mods, np, l - 1, batch, st);
}

hipError_t op_bfv_logic_gate(const Context& c, int gate, const u64* a, u64 as, const u64* b, int b_kind, u64 bs,
                             const u64* relin_key, u64* out, u64 so, int batch, u64* ws, hipStream_t st)
{
    if (batch <= 0) return hipSuccess; // an empty batch is a no-op, not an invalid launch
    int k[3];
    if (!logic_gate_coefficients(gate, k)) return hipErrorInvalidValue;
    const int np = c.n_power, Q = c.Q_size;
    const Mod* mods = c.plan_qp.mods;
    const u64* cd = c.tab.coeff_div_plain_modulus;
    const BfvPlainScale scale = bfv_plain_scale(c);
    if (gate == LOGIC_NOT)
        return rns_gate_combine(true, k[0], k[1], k[2], a, as, Q, nullptr, GATE_B_NONE, 0, 0, nullptr, 0, 0, 0.0, cd, scale,
                                out, so, mods, np, Q, batch, st);
    if (b_kind != GATE_B_CIPHER && b_kind != GATE_B_PLAIN) return hipErrorInvalidValue;
    const GateWs w = gate_ws(c, true, 0, batch);
    u64* prod = ws;
    u64* ks = ws + w.ks;
    if (b_kind == GATE_B_CIPHER) {
        TRY(op_bfv_multiply(c, a, as, b, bs, prod, w.ps, batch, ks, st));
        TRY(op_bfv_relinearize(c, prod, w.ps, relin_key, batch, ks, st));
    } else {
        for (int i = 0; i < batch; i++) // multiply_plain_bfv takes one ciphertext
            TRY(op_bfv_multiply_plain(c, a + as * i, b + bs * i, prod + w.ps * i, ks, st));
    }
    return rns_gate_combine(true, k[0], k[1], k[2], a, as, Q, b, b_kind, bs, Q, prod, w.ps, Q, 0.0, cd, scale, out, so, mods,
                            np, Q, batch, st);
}

// ------------------------------------------------------------------ keygen / encrypt / decrypt
// The plain transforms of this half: `polys` contiguous polynomials, polynomial i under modulus i % mod_count of table
// set `tables` (0: Q', 2: the plain modulus)
static hipError_t transform(const Context& c, const u64* in, u64* out, int mod_count, int polys, bool inverse,
                            hipStream_t st, int tables = 0)
{
    NttArgs a = c.ntt_args(tables);
    a.in = in; a.out = out; a.mod_count = mod_count;
    return ntt_launch(a, polys, inverse, st);
}
// ... and `batch` items of `limbs` polynomials each, item b at in + b * in_stride / out + b * out_stride; limb j under
// modulus j, or mod_order[j]
static hipError_t transform_items(const Context& c, const u64* in, u64 in_stride, u64* out, u64 out_stride, int limbs,
                                  int batch, bool inverse, hipStream_t st, const int* mod_order = nullptr)
{
    NttArgs a = c.ntt_args(0);
    a.in = in; a.out = out; a.mod_count = limbs; a.mod_order = mod_order;
    a.polys_per_item = limbs; a.in_item_stride = in_stride; a.out_item_stride = out_stride;
    return ntt_launch(a, batch * limbs, inverse, st);
}

hipError_t op_gen_secret_key(const Context& c, Rng& r, int hamming_weight, u64* sk, u64* ws, hipStream_t st)
{
    const int n = (int) c.n;
    if (hamming_weight <= 0 || hamming_weight > n) return hipErrorInvalidValue;
    // partial Fisher-Yates over the coefficient indices (the reference's v2 generator
    // does the same on the host with mt19937, ckks/keygenerator.cu:100-118)
    std::vector<int> index(n), host(2 * (size_t) hamming_weight);
    for (int i = 0; i < n; i++) index[i] = i;
    const u64 stream = r.stream++;
    for (int i = 0; i < hamming_weight; i++) {
        const DrbgOut o = drbg_block(r.seed, stream, (u64) i);
        const int j = i + (int) (((u64) o.w[0] * (u64) (n - i)) >> 32);
        std::swap(index[i], index[j]);
        host[i] = index[i];
        host[hamming_weight + i] = (o.w[1] & 1) ? 1 : -1;
    }
    int* dpos = reinterpret_cast<int*>(ws);
    TRY(hipMemcpyAsync(dpos, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, st));
    TRY(hipStreamSynchronize(st)); // the staging vector dies with this call
    TRY(kg_secret_rns(dpos, dpos + hamming_weight, hamming_weight, sk, c.plan_qp.mods, c.n_power, c.Qp_size, st));
    return transform(c, sk, sk, c.Qp_size, c.Qp_size, false, st);
}

// The single-party keys are the parties' shares with one generator in both roles: `a` first, then the errors
hipError_t op_gen_public_key(const Context& c, Rng& r, const u64* sk, u64* pk, u64* ws, hipStream_t st)
{
    return op_mpc_public_key_share(c, r, r, sk, pk, ws, st);
}

hipError_t op_gen_switch_key(const Context& c, Rng& r, const u64* sk, int galois_elt, const u64* old_sk, u64* key,
                             u64* ws, hipStream_t st)
{
    return op_mpc_switch_key_share(c, r, r, sk, galois_elt, nullptr, key, ws, st, old_sk);
}

// (pk*u + e) / P with rounding: the common front of both encryptions (encryptor.cu:52-100)
static hipError_t encrypt_zero(const Context& c, Rng& r, const u64* pk, u64* ct, u64* ws, hipStream_t st)
{
    const int np = c.n_power, Qp = c.Qp_size;
    const EncryptWs w = encrypt_ws(c);
    u64* u = ws;           // [Q'][N]
    u64* e = ws + w.e;     // [2][Q'][N]
    u64* pku = ws + w.pku; // [2][Q'][N]
    const Mod* mods = c.plan_qp.mods;
    TRY(kg_ternary(u, mods, np, Qp, 1, r.seed, r.stream++, st));
    TRY(kg_gaussian(e, mods, np, Qp, 2, r.seed, r.stream++, c.gauss_cdt, st));
    TRY(transform(c, u, u, Qp, Qp, false, st));
    TRY(kg_pk_u(pk, u, pku, mods, np, Qp, st));
    TRY(transform(c, pku, pku, Qp, 2 * Qp, true, st));
    TRY(rns_addition(pku, e, pku, mods, np, Qp, 2, 1, 0, st));
    return rns_moddown_extended(pku, 0, nullptr, 0, ct, 0, c.moddown(0), 0, 1, st);
}

hipError_t op_ckks_encrypt(const Context& c, Rng& r, const u64* pk, const u64* plain, u64* ct, u64* ws,
                           hipStream_t st)
{
    TRY(encrypt_zero(c, r, pk, ct, ws, st));                                               // :52-100
    TRY(transform(c, ct, ct, c.Q_size, 2 * c.Q_size, false, st));                          // :103
    return kg_message_add(ct, plain, c.plan_qp.mods, c.n_power, c.Q_size, st);             // :107
}

BfvPlainScale bfv_plain_scale(const Context& c)
{
    return BfvPlainScale{c.hv.Q_mod_t, c.hv.upper_threshold, c.plain_modulus};
}

hipError_t op_bfv_encrypt(const Context& c, Rng& r, const u64* pk, const u64* plain, u64* ct, u64* ws,
                          hipStream_t st)
{
    TRY(encrypt_zero(c, r, pk, ct, ws, st));
    return kg_bfv_message_add(ct, plain, c.plan_qp.mods, c.tab.coeff_div_plain_modulus, bfv_plain_scale(c), c.n_power,
                              c.Q_size, st);
}

static BfvDecryptDev bfv_decrypt_dev(const Context& c)
{
    BfvDecryptDev d{};
    d.plain = make_mod(c.plain_modulus);
    d.gamma = make_mod(c.hv.gamma);
    d.Qi_t = c.tab.Qi_t; d.Qi_gamma = c.tab.Qi_gamma; d.Qi_inverse = c.tab.Qi_inverse;
    d.mulq_inv_t = c.hv.mulq_inv_t;
    d.mulq_inv_gamma = c.hv.mulq_inv_gamma;
    d.inv_gamma = c.hv.inv_gamma;
    return d;
}

hipError_t op_bfv_decrypt(const Context& c, const u64* ct, const u64* sk, u64* plain, u64* ws, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    const u64* ct1 = ct + ((u64) Q << np);
    u64* t1 = ws; // [Q][N]
    TRY(transform(c, ct1, t1, Q, Q, false, st));                                           // :62
    TRY(kg_sk_multiplication(t1, sk, t1, c.plan_qp.mods, np, Q, st));                      // :65
    TRY(transform(c, t1, t1, Q, Q, true, st));                                             // :101
    return kg_bfv_decryption(ct, t1, plain, c.plan_qp.mods, bfv_decrypt_dev(c), np, Q, st); // :107
}

hipError_t op_bfv_noise_rns(const Context& c, const u64* ct, const u64* sk, u64* out, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    TRY(transform(c, ct + ((u64) Q << np), out, Q, Q, false, st));
    TRY(kg_sk_multiplication(out, sk, out, c.plan_qp.mods, np, Q, st));
    TRY(transform(c, out, out, Q, Q, true, st));
    return kg_coeff_multadd(ct, out, out, c.plain_modulus, c.plan_qp.mods, np, Q, st);
}

hipError_t op_bfv_encode(const Context& c, const long long* message, int message_size, u64* plain, hipStream_t st)
{
    if (!c.plan_plain.count) return hipErrorNotSupported;
    if (message_size < 0 || message_size > (int) c.n) return hipErrorInvalidValue;
    TRY(kg_bfv_encode_scatter(plain, message, c.tab.encoding_location, c.plain_modulus, message_size, c.n_power,
                              st));                                                        // :66
    return transform(c, plain, plain, 1, 1, true, st, 2);                                  // :81
}

hipError_t op_bfv_decode(const Context& c, const u64* plain, u64* message, u64* ws, hipStream_t st)
{
    if (!c.plan_plain.count) return hipErrorNotSupported;
    TRY(transform(c, plain, ws, 1, 1, false, st, 2));                                      // :234
    return kg_bfv_decode_gather(message, ws, c.tab.encoding_location, c.n_power, st);   // :239
}

hipError_t op_bfv_multiply_plain(const Context& c, const u64* ct, const u64* plain, u64* out, u64* ws, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    u64* pl = ws; // [Q][N]
    TRY(kg_bfv_threshold(plain, pl, c.plan_qp.mods, c.tab.upper_halfincrement, c.hv.upper_threshold, np, Q,
                         st));                                                             // :454
    TRY(transform(c, pl, pl, Q, Q, false, st));                                            // :479
    TRY(transform(c, ct, out, Q, 2 * Q, false, st));                                       // :484
    TRY(kg_pk_u(out, pl, out, c.plan_qp.mods, np, Q, st));                                 // :489 cipherplain_kernel
    return transform(c, out, out, Q, 2 * Q, true, st);                                     // :496
}

// HEOperator<BFV>::transform_to_ntt_bfv_plain (bfv/operator.cu:1398-1431): threshold lift mod every q_j, forward NTT
hipError_t op_bfv_plain_to_ntt(const Context& c, const u64* plain, u64* out, hipStream_t st)
{
    TRY(kg_bfv_threshold(plain, out, c.plan_qp.mods, c.tab.upper_halfincrement, c.hv.upper_threshold,
                         c.n_power, c.Q_size, st));
    return transform(c, out, out, c.Q_size, c.Q_size, false, st);
}

static int log2i(u64 v)
{
    int r = 0;
    while ((1ull << r) < v) r++;
    return r;
}

// mode: 0 real slots, 1 complex slots ((re, im) pairs), 2 polynomial coefficients, 3 one value in every slot
// (message == host pointer to that value is NOT used: the value comes in `scalar`)
hipError_t op_ckks_encode(const Context& c, int mode, const double* message, int message_size, double scalar,
                          double scale, u64* plain, u64* ws, hipStream_t st)
{
    const int slots = (int) (c.n >> 1), Q = c.Q_size;
    if (mode == 3)                                                                         // encoder.cu:412-446
        return en_coeff_conversion(plain, nullptr, 0, true, scalar * scale, c.plan_qp.mods, Q, c.n_power, st);
    if (mode == 2) {                                                                       // :222-261
        if (message_size < 0 || message_size > (int) c.n) return hipErrorInvalidValue;
        TRY(en_coeff_conversion(plain, message, message_size, false, scale, c.plan_qp.mods, Q, c.n_power, st));
        return transform(c, plain, plain, Q, Q, false, st);
    }
    if (message_size < 0 || message_size > slots) return hipErrorInvalidValue;
    void* cbuf = ws; // slots complex doubles = N words
    const double fix = scale / (double) slots;                                             // :127
    // double -> complex (:120) in the transform's first load
    TRY(en_special_fft(cbuf, c.tab.special_ifft_roots_table, log2i(slots), true, fix, st, message, message_size, mode == 1));
    TRY(en_conversion(plain, cbuf, c.plan_qp.mods, Q, c.tab.reverse_order, c.n_power, st)); // :138
    return transform(c, plain, plain, Q, Q, false, st);                                    // :153
}

// The decoder's CRT tables at a depth (ckks/decoder.cu:474-482): rows of Q, Q - 1, ... entries, Mi rows of their squares
struct DecoderTables {
    const u64 *Mi_inv, *Mi, *upper_half, *M;
};
static DecoderTables decoder_tables(const Context& c, int depth)
{
    const int loc1 = triangle_offset(c.Q_size, depth);
    int loc2 = 0;
    for (int i = 0; i < depth; i++) loc2 += (c.Q_size - i) * (c.Q_size - i);
    return {c.tab.Mi_inv + loc1, c.tab.Mi + loc2, c.tab.upper_half_threshold + loc1, c.tab.decryption_modulus + loc1};
}

// mode: 0 the N/2 real parts, 1 the N/2 complex slots, 2 the N coefficients
hipError_t op_ckks_decode(const Context& c, int mode, const u64* plain, int depth, double scale, double* message,
                          u64* ws, hipStream_t st)
{
    const int slots = (int) (c.n >> 1), l = c.Q_size - depth;
    if (l < 1) return hipErrorInvalidValue;
    u64* coeff = ws;                                   // [l][N]
    void* cbuf = ws + ckks_decode_ws(c, depth).second; // slots complex doubles
    TRY(transform(c, plain, coeff, l, l, true, st));                                       // :469
    const DecoderTables d = decoder_tables(c, depth);
    if (mode == 2)                                                                         // :586-635
        return en_coeff_compose(message, coeff, c.plan_qp.mods, d.Mi_inv, d.Mi, d.upper_half, d.M, l, scale, c.n_power,
                                st);
    TRY(en_compose(cbuf, coeff, c.plan_qp.mods, d.Mi_inv, d.Mi, d.upper_half, d.M, l, scale, c.tab.reverse_order,
                   c.n_power, st));                                                        // :485
    // :502, complex -> double (:505) in the transform's last store
    return en_special_fft(cbuf, c.tab.special_fft_roots_table, log2i(slots), false, 1.0, st, nullptr, 0, 0, message, mode == 1);
}

hipError_t op_ckks_decrypt(const Context& c, const u64* ct, const u64* sk, int depth, u64* plain, hipStream_t st)
{
    const int l = c.Q_size - depth;
    if (l < 1) return hipErrorInvalidValue;
    return kg_sk_multiplication_ckks(ct, plain, sk, c.plan_qp.mods, c.n_power, l, st);
}

// ------------------------------------------------------------------ N-out-of-N multiparty protocol
// `crs` is the generator every party seeds identically (the common `a` polynomials, public); `r` is the party's own.
// Both advance by one stream id per sampling call, so parties that make the same calls in the same order draw the
// same `a`.
int switch_key_digits(const Context& c) { return c.P_size == 1 ? c.Q_size : c.m2_levels[0].d; }

hipError_t op_mpc_public_key_share(const Context& c, Rng& crs, Rng& r, const u64* sk, u64* share, u64* ws,
                                   hipStream_t st)
{
    const int Qp = c.Qp_size;
    u64* e = ws;
    u64* av = ws + public_key_share_ws(c).second;
    TRY(kg_uniform(av, c.plan_qp.mods, c.n_power, Qp, 1, crs.seed, crs.stream++, st));
    TRY(kg_gaussian(e, c.plan_qp.mods, c.n_power, Qp, 1, r.seed, r.stream++, c.gauss_cdt, st));
    TRY(transform(c, e, e, Qp, Qp, false, st));
    return kg_publickey(share, sk, e, av, c.plan_qp.mods, c.n_power, Qp, st);
}

hipError_t op_mpc_switch_key_share(const Context& c, Rng& crs, Rng& r, const u64* sk, int galois_elt, u64* u_out,
                                   u64* share, u64* ws, hipStream_t st, const u64* old_sk)
{
    // method I: one digit per ciphertext prime; method II: the depth-0 digit partition
    // (ckks/keygenerator.cu:326-414 uses d_leveled[0] and Sk_pair_leveled[0])
    const int Q = c.Q_size, Qp = c.Qp_size, d = switch_key_digits(c);
    const int width = c.P_size == 1 ? 1 : c.m2_width;
    const int errs = u_out ? 2 : 1; // round 1 of the relinearisation key carries an error in both parts
    u64* e = ws;                                        // [errs][d][Q'][N]
    u64* av = ws + switch_key_share_ws(c, errs).second; // [d][Q'][N]
    const Mod* mods = c.plan_qp.mods;
    TRY(kg_uniform(av, mods, c.n_power, Qp, d, crs.seed, crs.stream++, st));
    TRY(kg_gaussian(e, mods, c.n_power, Qp, errs * d, r.seed, r.stream++, c.gauss_cdt, st));
    TRY(transform(c, e, e, Qp, errs * d * Qp, false, st));
    if (u_out) {
        TRY(kg_ternary(u_out, mods, c.n_power, Qp, 1, r.seed, r.stream++, st));
        TRY(transform(c, u_out, u_out, Qp, Qp, false, st));
    }
    const int inv = galois_elt ? (int) inv_mod_2n((u64) galois_elt, 2 * c.n) : 0; // keygenerator.cu:474
    return kg_switchkey(share, sk, e, av, mods, c.tab.factor, inv, old_sk, c.n_power, Qp, d, width, Q, c.P_size, st,
                        u_out, u_out ? e + (u64) d * Qp * c.n : nullptr);
}

hipError_t op_mpc_relin_key_share_round2(const Context& c, Rng& r, const u64* sk, const u64* u, const u64* round1_sum,
                                         u64* share, u64* ws, hipStream_t st)
{
    const int Qp = c.Qp_size, d = switch_key_digits(c);
    u64* e = ws; // [2][d][Q'][N], the first region of switch_key_share_ws(c, 2)
    TRY(kg_gaussian(e, c.plan_qp.mods, c.n_power, Qp, 2 * d, r.seed, r.stream++, c.gauss_cdt, st));
    TRY(transform(c, e, e, Qp, 2 * d * Qp, false, st));
    return kg_mpc_relin_round2(share, round1_sum, sk, u, e, c.plan_qp.mods, c.n_power, Qp, d, st);
}

hipError_t op_mpc_accumulate(const Context& c, const u64* const* shares, int k, int layout, const u64* round1_sum,
                             u64* out, hipStream_t st)
{
    const int units = layout == MPC_LAYOUT_PUBLIC_KEY ? 1 : switch_key_digits(c);
    const bool finish = layout == MPC_LAYOUT_RELIN_FINISH;
    return kg_mpc_accumulate(out, shares, k, finish ? round1_sum : shares[0], finish, layout == MPC_LAYOUT_RELIN_ROUND1,
                             c.plan_qp.mods, c.n_power, c.Qp_size, units, st);
}

hipError_t op_mpc_ckks_decrypt_share(const Context& c, Rng& r, const u64* ct, u64 cs, const u64* sk, int depth,
                                     u64* share, int batch, hipStream_t st)
{
    const int l = c.Q_size - depth;
    const Mod* mods = c.plan_qp.mods;
    TRY(kg_gaussian(share, mods, c.n_power, l, batch, r.seed, r.stream++, c.gauss_cdt, st));   // :1510
    TRY(transform(c, share, share, l, batch * l, false, st));                                  // :1524
    return kg_mpc_share(share, ct + ((u64) l << c.n_power), cs, sk, mods, c.n_power, l, 0, batch, DrbgKey{}, 0, 1, st);
}

hipError_t op_mpc_bfv_decrypt_share(const Context& c, Rng& r, const u64* ct, u64 cs, const u64* sk, u64* share,
                                    int batch, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    const Mod* mods = c.plan_qp.mods;
    TRY(transform_items(c, ct + ((u64) Q << np), cs, share, (u64) Q << np, Q, batch, false, st)); // :1461
    TRY(kg_mpc_share(share, share, (u64) Q << np, sk, mods, np, Q, 0, batch, DrbgKey{}, 0, 0, st)); // :1465
    TRY(transform(c, share, share, Q, batch * Q, true, st));                                   // :1492
    return kg_mpc_add_gaussian(share, mods, np, Q, batch, r.seed, r.stream++, c.gauss_cdt, st); // :1499-1510
}

hipError_t op_mpc_ckks_decrypt_merge(const Context& c, const u64* ct, u64 cs, const u64* const* shares, int k,
                                     int depth, u64* plain, int batch, hipStream_t st)
{
    const int l = c.Q_size - depth;
    const u64 stride = (u64) l << c.n_power;
    return kg_mpc_sum(plain, stride, ct, cs, shares, k, stride, 0, c.plan_qp.mods, c.n_power, l, batch, st);
}

// plain [batch][N] = scale-and-round(c0 + the sum of the k shares, items sh_stride apart).  The rounding kernel takes one
// group of shares: everything but the last group is summed into head_sum [batch][Q][N] first.
static hipError_t bfv_sum_and_round(const Context& c, const u64* ct, u64 cs, const u64* const* shares, int k,
                                    u64 sh_stride, u64* plain, u64* head_sum, int batch, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    const Mod* mods = c.plan_qp.mods;
    const int head = (k - 1) / KG_MPC_MAX_SHARES * KG_MPC_MAX_SHARES;
    if (head) {
        const u64 part = (u64) Q << np;
        TRY(kg_mpc_sum(head_sum, part, ct, cs, shares, head, sh_stride, 0, mods, np, Q, batch, st));
        ct = head_sum;
        cs = part;
    }
    return kg_mpc_bfv_round(plain, ct, cs, shares + head, k - head, sh_stride, mods, bfv_decrypt_dev(c), np, Q, batch, st);
}

hipError_t op_mpc_bfv_decrypt_merge(const Context& c, const u64* ct, u64 cs, const u64* const* shares, int k,
                                    u64* plain, int batch, u64* ws, hipStream_t st)
{
    return bfv_sum_and_round(c, ct, cs, shares, k, (u64) c.Q_size << c.n_power, plain, ws, batch, st);
}

// ------------------------------------------------------------------ collective refresh
int level_modulus_bits(const Context& c, int l)
{
    std::vector<u64> big{1};
    for (int j = 0; j < l; j++) {
        unsigned __int128 carry = 0;
        for (u64& w : big) {
            const unsigned __int128 v = (unsigned __int128) w * c.primes[j] + carry;
            w = (u64) v;
            carry = v >> 64;
        }
        if (carry) big.push_back((u64) carry);
    }
    return 64 * (int) (big.size() - 1) + (64 - __builtin_clzll(big.back()));
}

// the first of `count` stream ids, one per item of the batch
static u64 take_streams(Rng& r, int count)
{
    const u64 first = r.stream;
    r.stream += (u64) count;
    return first;
}

hipError_t op_mpc_ckks_refresh_share(const Context& c, Rng& crs, Rng& r, const u64* ct, u64 cs, const u64* sk,
                                     int depth, int mask_bits, u64* share, int batch, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size, l = Q - depth;
    const Mod* mods = c.plan_qp.mods;
    TRY(kg_mpc_refresh_noise(share, mods, np, l, Q, batch, r.seed, r.stream, c.gauss_cdt, mask_bits, st));
    r.stream += 3 * (u64) batch;
    const u64 sh_stride = (u64) (l + Q) << np;
    // one transform over both halves: moduli 0..l-1, then 0..Q-1
    TRY(transform_items(c, share, sh_stride, share, sh_stride, l + Q, batch, false, st,
                        c.tab.mpc_refresh_order + (depth * 2 * Q - depth * (depth - 1) / 2)));
    return kg_mpc_share(share, ct + ((u64) l << np), cs, sk, mods, np, l, Q, batch, crs.seed, take_streams(crs, batch), 1,
                        st);
}

hipError_t op_mpc_ckks_refresh_merge(const Context& c, Rng& crs, const u64* ct, u64 cs, const u64* const* shares,
                                     int k, int depth, u64* out, u64 so, int batch, u64* ws, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size, l = Q - depth;
    const Mod* mods = c.plan_qp.mods;
    const u64 sh_stride = (u64) (l + Q) << np, t_stride = (u64) l << np;
    u64* t = ws; // [batch][l][N]
    TRY(kg_mpc_sum(t, t_stride, ct, cs, shares, k, sh_stride, 0, mods, np, l, batch, st));
    TRY(transform(c, t, t, l, batch * l, true, st));
    const DecoderTables d = decoder_tables(c, depth);
    TRY(kg_mpc_refresh_lift(out, so, t, mods, d.Mi_inv, d.Mi, d.upper_half, d.M, l, Q, np, batch, st));
    TRY(transform_items(c, out, so, out, so, Q, batch, false, st));
    return kg_mpc_refresh_finish(out, so, shares, k, sh_stride, t_stride, 1, nullptr, nullptr, BfvPlainScale{}, mods,
                                 np, Q, batch, crs.seed, take_streams(crs, batch), st);
}

hipError_t op_mpc_bfv_refresh_share(const Context& c, Rng& crs, Rng& r, const u64* ct, u64 cs, const u64* sk,
                                    u64* share, int batch, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    const Mod* mods = c.plan_qp.mods;
    const u64 sh_stride = (u64) (2 * Q) << np;
    TRY(transform_items(c, ct + ((u64) Q << np), cs, share, sh_stride, Q, batch, false, st));
    TRY(kg_mpc_share(share, share, sh_stride, sk, mods, np, Q, Q, batch, crs.seed, take_streams(crs, batch), 0, st));
    TRY(transform(c, share, share, Q, batch * 2 * Q, true, st));
    TRY(kg_mpc_refresh_bfv_noise(share, mods, c.tab.coeff_div_plain_modulus, bfv_plain_scale(c), np, Q, batch, r.seed,
                                 r.stream, c.gauss_cdt, st));
    r.stream += 3 * (u64) batch;
    return hipSuccess;
}

hipError_t op_mpc_bfv_refresh_merge(const Context& c, Rng& crs, const u64* ct, u64 cs, const u64* const* shares,
                                    int k, u64* out, u64 so, int batch, u64* ws, hipStream_t st)
{
    const int np = c.n_power, Q = c.Q_size;
    const Mod* mods = c.plan_qp.mods;
    const u64 sh_stride = (u64) (2 * Q) << np, part = (u64) Q << np;
    u64* plain = ws;                                              // [batch][N]
    u64* head_sum = ws + bfv_refresh_merge_ws(c, batch).head_sum; // [batch][Q][N], beyond 16 shares
    TRY(bfv_sum_and_round(c, ct, cs, shares, k, sh_stride, plain, head_sum, batch, st));
    TRY(kg_mpc_refresh_finish(out, so, shares, k, sh_stride, part, 0, plain, c.tab.coeff_div_plain_modulus,
                              bfv_plain_scale(c), mods, np, Q, batch, crs.seed, take_streams(crs, batch), st));
    return transform_items(c, out + part, so, out + part, so, Q, batch, true, st); // c1' = INTT(a)
}

} // namespace hegpu
