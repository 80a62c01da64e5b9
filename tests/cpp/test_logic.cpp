// Logic gates on encrypted bits through the class layer (include/heongpu/heongpu.hpp: HELogicOperator<Scheme::BFV> and
// HELogicOperator<Scheme::CKKS>): every gate with a ciphertext and with a plaintext second operand, out of place and in
// place, on the four input pairs; the result's depth_, scale_ and flags; the exception type of every refusal; a HOST-stored
// operand through the storage manager; the input of an out-of-place NOT left as it was.  A CKKS bit is right when it rounds
// to the table's value (error below 0.5).  Exits non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc logictest`.
#include <heongpu/heongpu.hpp>

#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

using namespace heongpu;

static int failures = 0;
#define EXPECT(cond, what)                                   \
    do {                                                     \
        if (!(cond)) { failures++; std::printf("FAIL: %s\n", what); } \
        else std::printf("ok:   %s\n", what);                \
    } while (0)

template <typename E, typename F> static bool throws(F&& f)
{
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

static const char* kNames[6] = {"AND", "OR", "XOR", "NAND", "NOR", "XNOR"};
static int table(int g, int x, int y)
{
    switch (g) {
        case 0: return x & y;
        case 1: return x | y;
        case 2: return x ^ y;
        case 3: return 1 - (x & y);
        case 4: return 1 - (x | y);
        default: return 1 - (x ^ y);
    }
}

template <Scheme S> struct Forms {
    using Op = HELogicOperator<S>;
    std::function<void(Op&, Ciphertext<S>&, Ciphertext<S>&, Ciphertext<S>&, Relinkey<S>&)> cc;
    std::function<void(Op&, Ciphertext<S>&, Ciphertext<S>&, Relinkey<S>&)> cc_in;
    std::function<void(Op&, Ciphertext<S>&, Plaintext<S>&, Ciphertext<S>&)> cp;
    std::function<void(Op&, Ciphertext<S>&, Plaintext<S>&)> cp_in;
};
#define FORMS(S, NAME)                                                                                                  \
    Forms<S>{[](HELogicOperator<S>& o, Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& r, Relinkey<S>& k) { o.NAME(a, b, r, k); }, \
             [](HELogicOperator<S>& o, Ciphertext<S>& a, Ciphertext<S>& b, Relinkey<S>& k) { o.NAME##_inplace(a, b, k); },  \
             [](HELogicOperator<S>& o, Ciphertext<S>& a, Plaintext<S>& b, Ciphertext<S>& r) { o.NAME(a, b, r); },           \
             [](HELogicOperator<S>& o, Ciphertext<S>& a, Plaintext<S>& b) { o.NAME##_inplace(a, b); }}
template <Scheme S> static std::vector<Forms<S>> all_forms()
{
    return {FORMS(S, AND), FORMS(S, OR), FORMS(S, XOR), FORMS(S, NAND), FORMS(S, NOR), FORMS(S, XNOR)};
}

static void bfv()
{
    constexpr auto S = Scheme::BFV;
    const size_t n = 4096;
    HEContext<S> ctx = GenHEContext<S>();
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_default_values(1);
    ctx->set_plain_modulus(65537);
    ctx->generate();
    HEKeyGenerator<S> keygen(ctx);
    Secretkey<S> sk(ctx);
    keygen.generate_secret_key(sk);
    Publickey<S> pk(ctx);
    keygen.generate_public_key(pk, sk);
    Relinkey<S> rk(ctx);
    keygen.generate_relin_key(rk, sk);
    HEEncoder<S> encoder(ctx);
    HEEncryptor<S> enc(ctx, pk);
    HEDecryptor<S> dec(ctx, sk);
    HELogicOperator<S> op(ctx, encoder);
    HEArithmeticOperator<S> arith(ctx, encoder);

    std::vector<uint64_t> x(n), y(n);
    for (size_t i = 0; i < n; i++) { x[i] = (i >> 1) & 1; y[i] = i & 1; }
    Plaintext<S> px(ctx), py(ctx);
    encoder.encode(px, x);
    encoder.encode(py, y);
    Ciphertext<S> cx(ctx), cy(ctx);
    enc.encrypt(cx, px);
    enc.encrypt(cy, py);

    auto bits = [&](Ciphertext<S>& c) {
        Plaintext<S> p(ctx);
        dec.decrypt(p, c);
        std::vector<uint64_t> v;
        encoder.decode(v, p);
        return v;
    };
    auto is_gate = [&](Ciphertext<S>& c, int g) {
        const std::vector<uint64_t> v = bits(c);
        bool ok = v.size() == n;
        for (size_t i = 0; ok && i < n; i++) ok = v[i] == (uint64_t) (g < 0 ? 1 - (int) x[i] : table(g, (int) x[i], (int) y[i]));
        return ok && c.size() == 2 && !c.relinearization_required() && !c.in_ntt_domain();
    };

    const auto forms = all_forms<S>();
    bool ok_cc = true, ok_cc_in = true, ok_cp = true, ok_cp_in = true;
    for (int g = 0; g < 6; g++) {
        Ciphertext<S> r(ctx), a1 = cx, a2 = cx;
        forms[g].cc(op, cx, cy, r, rk);
        if (!is_gate(r, g)) { ok_cc = false; std::printf("  BFV %s (ct, ct) wrong\n", kNames[g]); }
        forms[g].cc_in(op, a1, cy, rk);
        if (!is_gate(a1, g)) { ok_cc_in = false; std::printf("  BFV %s_inplace (ct, ct) wrong\n", kNames[g]); }
        Ciphertext<S> r2(ctx);
        forms[g].cp(op, cx, py, r2);
        if (!is_gate(r2, g)) { ok_cp = false; std::printf("  BFV %s (ct, pt) wrong\n", kNames[g]); }
        forms[g].cp_in(op, a2, py);
        if (!is_gate(a2, g)) { ok_cp_in = false; std::printf("  BFV %s_inplace (ct, pt) wrong\n", kNames[g]); }
    }
    EXPECT(ok_cc, "BFV: the six gates on two ciphertexts give their truth tables");
    EXPECT(ok_cc_in, "BFV: ... in place");
    EXPECT(ok_cp, "BFV: the six gates on a ciphertext and a plaintext give their truth tables");
    EXPECT(ok_cp_in, "BFV: ... in place");

    std::vector<Data64> before, after;
    cx.get_data(before);
    Ciphertext<S> nx(ctx);
    op.NOT(cx, nx);
    cx.get_data(after);
    EXPECT(is_gate(nx, -1), "BFV: NOT gives 1 - x");
    EXPECT(before == after, "BFV: the input of an out-of-place NOT is unchanged");
    op.NOT_inplace(nx);
    {
        const std::vector<uint64_t> v = bits(nx);
        EXPECT(v == x, "BFV: NOT_inplace of NOT x is x");
    }

    // a HOST-stored operand is staged for the gate and goes back
    cy.store_in_host();
    EXPECT(!cy.is_on_device(), "BFV: an operand parked in host memory");
    Ciphertext<S> r(ctx);
    op.XOR(cx, cy, r, rk);
    EXPECT(is_gate(r, 2) && !cy.is_on_device() && r.is_on_device(), "BFV: XOR with a HOST-stored operand; it stays in host memory");
    cy.store_in_device();

    // refusals
    Ciphertext<S> prod(ctx);
    arith.multiply(cx, cy, prod);
    EXPECT(throws<std::invalid_argument>([&] { op.AND(prod, cy, r, rk); }) && throws<std::invalid_argument>([&] { op.NOT(prod, r); }),
           "BFV: a three-part input is std::invalid_argument");
    Ciphertext<S> cn(ctx);
    arith.transform_to_ntt(cx, cn);
    EXPECT(throws<std::invalid_argument>([&] { op.OR(cn, cy, r, rk); }) && throws<std::invalid_argument>([&] { op.OR(cx, cn, r, rk); }),
           "BFV: a ciphertext in the NTT domain is std::invalid_argument");
    Plaintext<S> pn(ctx);
    arith.transform_to_ntt(py, pn);
    EXPECT(throws<std::logic_error>([&] { op.OR(cx, pn, r); }), "BFV: a plaintext in the NTT domain is std::logic_error");
    Ciphertext<S> empty(ctx);
    EXPECT(throws<std::invalid_argument>([&] { op.NOR(empty, cy, r, rk); }) && throws<std::invalid_argument>([&] { op.NOT(empty, r); }),
           "BFV: undersized memory is std::invalid_argument");
}

static void ckks()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({50, 30, 30, 30}, {50});
    ctx->generate();
    const double scale = std::pow(2.0, 30);
    HEKeyGenerator<S> keygen(ctx);
    Secretkey<S> sk(ctx);
    keygen.generate_secret_key(sk);
    Publickey<S> pk(ctx);
    keygen.generate_public_key(pk, sk);
    Relinkey<S> rk(ctx);
    keygen.generate_relin_key(rk, sk);
    HEEncoder<S> encoder(ctx);
    HEEncryptor<S> enc(ctx, pk);
    HEDecryptor<S> dec(ctx, sk);
    HELogicOperator<S> op(ctx, encoder, scale);
    HEArithmeticOperator<S> arith(ctx, encoder);
    EXPECT(throws<std::invalid_argument>([&] { HELogicOperator<S> bad(ctx, encoder, 0.0); }),
           "CKKS: a zero scale is std::invalid_argument");

    std::vector<double> x(slots), y(slots);
    for (size_t i = 0; i < slots; i++) { x[i] = (double) ((i >> 1) & 1); y[i] = (double) (i & 1); }
    Plaintext<S> px(ctx), py(ctx);
    encoder.encode(px, x, scale);
    encoder.encode(py, y, scale);
    Ciphertext<S> cx(ctx), cy(ctx);
    enc.encrypt(cx, px);
    enc.encrypt(cy, py);
    const double q_last = (double) ctx->prime_vector_[3].value;

    double worst = 0;
    auto is_gate = [&](Ciphertext<S>& c, int g) {
        Plaintext<S> p(ctx);
        dec.decrypt(p, c);
        std::vector<double> v;
        encoder.decode(v, p);
        bool ok = v.size() >= slots;
        for (size_t i = 0; ok && i < slots; i++) {
            const int want = g < 0 ? 1 - (int) x[i] : table(g, (int) x[i], (int) y[i]);
            worst = std::max(worst, std::fabs(v[i] - want));
            ok = std::lround(v[i]) == want;
        }
        return ok;
    };
    auto meta = [&](Ciphertext<S>& c, int g) { // depth + 1, the product's scale for AND / NAND, flags cleared
        const double want = (g == 0 || g == 3) ? scale * scale / q_last : scale;
        return c.depth() == 1 && c.size() == 2 && !c.rescale_required() && !c.relinearization_required() &&
               std::fabs(c.scale() / want - 1.0) < 1e-12 && c.memory_size() == 2 * 3 * n;
    };

    const auto forms = all_forms<S>();
    bool ok_cc = true, ok_cc_in = true, ok_cp = true, ok_cp_in = true, ok_meta = true;
    for (int g = 0; g < 6; g++) {
        Ciphertext<S> r(ctx), a1 = cx, a2 = cx;
        forms[g].cc(op, cx, cy, r, rk);
        if (!is_gate(r, g)) { ok_cc = false; std::printf("  CKKS %s (ct, ct) wrong\n", kNames[g]); }
        forms[g].cc_in(op, a1, cy, rk);
        if (!is_gate(a1, g)) { ok_cc_in = false; std::printf("  CKKS %s_inplace (ct, ct) wrong\n", kNames[g]); }
        Ciphertext<S> r2(ctx);
        forms[g].cp(op, cx, py, r2);
        if (!is_gate(r2, g)) { ok_cp = false; std::printf("  CKKS %s (ct, pt) wrong\n", kNames[g]); }
        forms[g].cp_in(op, a2, py);
        if (!is_gate(a2, g)) { ok_cp_in = false; std::printf("  CKKS %s_inplace (ct, pt) wrong\n", kNames[g]); }
        if (!(meta(r, g) && meta(a1, g) && meta(r2, g) && meta(a2, g))) { ok_meta = false; std::printf("  CKKS %s metadata wrong\n", kNames[g]); }
    }
    EXPECT(ok_cc, "CKKS: the six gates on two ciphertexts round to their truth tables (OR, XOR, NOR, XNOR too)");
    EXPECT(ok_cc_in, "CKKS: ... in place");
    EXPECT(ok_cp, "CKKS: the six gates on a ciphertext and a plaintext round to their truth tables");
    EXPECT(ok_cp_in, "CKKS: ... in place");
    EXPECT(ok_meta, "CKKS: depth + 1, the product's scale for AND / NAND and the first operand's otherwise, flags cleared");

    std::vector<Data64> before, after;
    cx.get_data(before);
    Ciphertext<S> nx(ctx);
    op.NOT(cx, nx);
    cx.get_data(after);
    EXPECT(is_gate(nx, -1) && nx.depth() == 0 && nx.scale() == scale && nx.memory_size() == 2 * 4 * n,
           "CKKS: NOT gives 1 - x at the input's depth and scale");
    EXPECT(before == after, "CKKS: the input of an out-of-place NOT is unchanged");
    op.NOT_inplace(nx);
    {
        std::vector<double> keep = y;
        y.assign(slots, 0.0);
        EXPECT(is_gate(nx, 1), "CKKS: NOT_inplace of NOT x is x"); // x | 0
        y = keep;
    }
    std::printf("CKKS: largest |decoded - bit| over all gates = %.3e\n", worst);

    // the example's flow: a plaintext dropped to the level of a result, then a gate on both
    Ciphertext<S> c2(ctx);
    op.AND(cx, cx, c2, rk);
    Plaintext<S> ones(ctx);
    encoder.encode(ones, std::vector<double>(slots, 1.0), scale);
    op.mod_drop_inplace(ones);
    EXPECT(ones.depth() == 1, "CKKS: mod_drop_inplace of a plaintext through the logic operator");
    op.XNOR_inplace(c2, ones);
    {
        std::vector<double> keep = y;
        y.assign(slots, 1.0);
        EXPECT(is_gate(c2, 5) && c2.depth() == 2, "CKKS: XNOR(AND(x, x), 1) is x, two levels down");
        y = keep;
    }
    Ciphertext<S> low(ctx);
    op.mod_drop(cx, low);
    EXPECT(low.depth() == 1 && low.memory_size() == 2 * 3 * n, "CKKS: mod_drop of a ciphertext through the logic operator");

    // a HOST-stored operand is staged for the gate and goes back
    cy.store_in_host();
    Ciphertext<S> r(ctx);
    op.XOR(cx, cy, r, rk);
    EXPECT(is_gate(r, 2) && !cy.is_on_device() && r.is_on_device(), "CKKS: XOR with a HOST-stored operand; it stays in host memory");
    cy.store_in_device();

    // refusals
    EXPECT(throws<std::logic_error>([&] { op.OR(cx, low, r, rk); }) && throws<std::logic_error>([&] { op.OR(low, py, r); }),
           "CKKS: unequal depths are std::logic_error");
    Ciphertext<S> prod(ctx);
    arith.multiply(cx, cy, prod);
    EXPECT(throws<std::invalid_argument>([&] { op.AND(prod, cy, r, rk); }) && throws<std::invalid_argument>([&] { op.NOT(prod, r); }),
           "CKKS: a three-part input (relinearization pending) is std::invalid_argument");
    arith.relinearize_inplace(prod, rk);
    EXPECT(throws<std::invalid_argument>([&] { op.AND(cx, prod, r, rk); }) && throws<std::invalid_argument>([&] { op.NOT_inplace(prod); }),
           "CKKS: a pending rescale is std::invalid_argument");
    Ciphertext<S> empty(ctx);
    EXPECT(throws<std::invalid_argument>([&] { op.NOR(empty, cy, r, rk); }), "CKKS: undersized memory is std::invalid_argument");
    Ciphertext<S> last = low, tmp(ctx);
    for (int k = 0; k < 2; k++) { op.mod_drop(last, tmp); last = tmp; }
    EXPECT(last.depth() == 3 && throws<std::logic_error>([&] { op.AND(last, last, r, rk); }),
           "CKKS: a binary gate on the last level is std::logic_error");
    op.NOT(last, r);
    EXPECT(r.depth() == 3, "CKKS: NOT works on the last level");
}

int main()
{
    bfv();
    ckks();
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all logic class-layer checks passed\n");
    return 0;
}
