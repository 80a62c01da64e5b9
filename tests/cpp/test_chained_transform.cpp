// Chained giant steps through the class layer (include/heongpu/heongpu.hpp: LinearTransform's chain_giant_steps,
// HEArithmeticOperator::set_chained_giant_steps).
//   1. a LinearTransform with chain_giant_steps: required_shifts() holds the links in the place of the giant shifts, the
//      Galois key is built from them alone, and encrypt -> linear_transform -> rescale_inplace -> decrypt -> decode equals
//      the dense product under the reference tests' criterion |a - b| < 1e-4; the direct transform of the same matrix
//      does not run on that key (std::invalid_argument);
//   2. with the switch on, generate_encoding_transform_context yields a key_indexs_ that is smaller than, and a subset
//      of, the one with the switch off; a Galoiskey built from it carries coeff_to_slot -> slot_to_coeff on the
//      parameters of the reference's example under the example's own 5e-2; less_key_mode stays refused.
// Exits non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc chainedtransformtest`.
#include <heongpu/heongpu.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

using namespace heongpu;

static int failures = 0;
#define EXPECT(cond, what)                                   \
    do {                                                     \
        if (!(cond)) { failures++; std::printf("FAIL: %s\n", what); } \
        else std::printf("ok:   %s\n", what);                \
    } while (0)

template <typename F> static bool throws_invalid(F&& f)
{
    try { f(); } catch (const std::invalid_argument&) { return true; } catch (...) { return false; }
    return false;
}

static bool subset(const std::vector<int>& a, const std::vector<int>& b)
{
    return std::all_of(a.begin(), a.end(), [&](int x) { return std::find(b.begin(), b.end(), x) != b.end(); });
}

static void matrix_times_vector()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({60, 40, 40}, {60});
    ctx->generate();
    HEEncoder<S> encoder(ctx);
    const int slots = encoder.slot_count();
    const double scale = std::pow(2.0, 40);
    std::mt19937_64 gen(7);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);

    const std::vector<int> ks{0, 1, 2, 3, 5, 8, 13, 21, 100, 2047};
    std::map<int, std::vector<double>> diag;
    for (int k : ks) {
        std::vector<double> d(slots);
        for (double& x : d) x = unit(gen);
        diag[k] = d;
    }
    std::vector<double> v(slots), want(slots, 0.0), got;
    for (double& x : v) x = unit(gen);
    for (int k : ks)
        for (int s = 0; s < slots; s++) want[s] += diag[k][s] * v[(s + k) % slots];

    LinearTransform<S> direct(ctx, diag, encoder, scale);
    LinearTransform<S> lt(ctx, diag, encoder, scale, 0, 0, ExecutionOptions(), 1, true);
    EXPECT(!direct.chained() && direct.giant_parent() == nullptr && direct.link_shifts() == direct.giant_shifts(),
           "without chain_giant_steps a transform has no parent table and its links are its giant shifts");
    EXPECT(lt.chained() && lt.n1() == 4 && lt.n2() == 7 && lt.giant_shifts() == direct.giant_shifts() &&
               lt.index() == direct.index(),
           "the chained transform has the plan of the direct one");
    // giant shifts 0, 4, 8, 12, 20, 100, -4: links 0, 4, 4, 4, 8, 80, -4
    const std::vector<int> links{0, 4, 4, 4, 8, 80, slots - 4};
    EXPECT(lt.link_shifts() == links, "the links are the differences of neighbouring giant shifts");
    const std::vector<int> shifts = lt.required_shifts();
    EXPECT((shifts == std::vector<int>{1, 2, 3, 4, 8, 80, slots - 4}), "required_shifts: the baby shifts and the distinct links");
    EXPECT(shifts.size() < direct.required_shifts().size(), "fewer keys than the direct transform needs");

    HEKeyGenerator<S> keygen(ctx);
    Secretkey<S> sk(ctx);
    keygen.generate_secret_key(sk);
    Publickey<S> pk(ctx);
    keygen.generate_public_key(pk, sk);
    Galoiskey<S> gk(ctx, shifts);
    keygen.generate_galois_key(gk, sk);
    HEEncryptor<S> enc(ctx, pk);
    HEDecryptor<S> dec(ctx, sk);
    HEArithmeticOperator<S> op(ctx);

    Plaintext<S> pv(ctx), pr(ctx);
    encoder.encode(pv, v, scale);
    Ciphertext<S> cv(ctx), cy(ctx);
    enc.encrypt(cv, pv);
    op.linear_transform(cv, lt, gk, cy);
    EXPECT(cy.rescale_required() && cy.scale() == scale * scale && cy.depth() == 0, "the result awaits its rescale at scale^2");
    op.rescale_inplace(cy);
    dec.decrypt(pr, cy);
    encoder.decode(got, pr);
    double err = 0;
    for (int s = 0; s < slots; s++) err = std::max(err, std::fabs(got[s] - want[s]));
    std::printf("chained: max |decode - M v| = %.3e (criterion 1e-4)\n", err);
    EXPECT((int) got.size() == slots && err < 1e-4, "the chained transform of an encrypted vector is the matrix product");

    Ciphertext<S> cz(ctx);
    EXPECT(throws_invalid([&] { op.linear_transform(cv, direct, gk, cz); }),
           "the direct transform lacks keys in the reduced set: std::invalid_argument");
    Galoiskey<S> few(ctx, std::vector<int>{1, 2, 3, 4});
    keygen.generate_galois_key(few, sk);
    EXPECT(throws_invalid([&] { op.linear_transform(cv, lt, few, cz); }), "a link without its key is std::invalid_argument");
}

static void encoding_transforms()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({50, 40, 40, 40, 40, 40, 40, 40, 40}, {50});
    ctx->generate();
    const double scale = std::pow(2.0, 40);
    HEKeyGenerator<S> keygen(ctx);
    Secretkey<S> sk(ctx);
    keygen.generate_secret_key(sk);
    Publickey<S> pk(ctx);
    keygen.generate_public_key(pk, sk);
    HEEncoder<S> encoder(ctx);
    HEEncryptor<S> enc(ctx, pk);
    HEDecryptor<S> dec(ctx, sk);
    HEArithmeticOperator<S> op(ctx, encoder);

    CKKSEncodingTransformConfig config(3, 3, 0, 4, false);
    CKKSEncodingTransformContext direct, tc;
    EXPECT(!op.chained_giant_steps(), "the switch is off by default");
    op.generate_encoding_transform_context(direct, scale, config);
    op.set_chained_giant_steps(true);
    op.generate_encoding_transform_context(tc, scale, config);
    std::printf("rotation keys: direct %zu, chained %zu\n", direct.key_indexs_.size(), tc.key_indexs_.size());
    EXPECT(direct.key_indexs_.size() == 29 && tc.key_indexs_.size() == 18, "29 rotation keys direct, 18 chained (N = 2^12, 3 + 3)");
    EXPECT(subset(tc.key_indexs_, direct.key_indexs_), "the chained key set is a subset of the direct one");
    EXPECT(!tc.less_key_mode_, "less_key_mode_ keeps the reference's meaning and stays false");
    CKKSEncodingTransformContext t2;
    EXPECT(throws_invalid([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 0, 4, true}); }) && !t2.generated_,
           "less_key_mode stays std::invalid_argument with the switch on");

    Galoiskey<S> gk(ctx, tc.key_indexs_);
    keygen.generate_galois_key(gk, sk);
    std::vector<double> message(n);
    std::mt19937_64 gen(3);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    for (double& x : message) x = unit(gen);
    Plaintext<S> plain(ctx);
    encoder.encode(plain, message, scale, ExecutionOptions(), encoding::COEFFICIENT);
    Ciphertext<S> cipher(ctx);
    enc.encrypt(cipher, plain);
    std::vector<Ciphertext<S>> pair = op.coeff_to_slot(cipher, gk, tc);
    EXPECT(pair.size() == 2 && pair[0].depth() == 4 && pair[1].depth() == 4, "three pieces from level 0 leave at level 4");
    Ciphertext<S> back = op.slot_to_coeff(pair[0], pair[1], gk, tc);
    EXPECT(back.depth() == 8, "three pieces from level 4 leave at level 8");
    Plaintext<S> p_ref(ctx), p_back(ctx);
    dec.decrypt(p_ref, cipher);
    dec.decrypt(p_back, back);
    std::vector<double> ref, got;
    encoder.decode(ref, p_ref);
    encoder.decode(got, p_back);
    double e_round = 0;
    for (size_t k = 0; k < n; k++) e_round = std::max(e_round, std::fabs(ref[k] - got[k]));
    std::printf("chained: max |round trip - input| = %.3e (criterion 5e-2)\n", e_round);
    EXPECT(ref.size() == n && got.size() == n && e_round < 5e-2, "slot_to_coeff(coeff_to_slot(x)) = x on the reduced keys");
    EXPECT(throws_invalid([&] { op.coeff_to_slot(cipher, gk, direct); }),
           "the direct context does not run on the reduced keys: std::invalid_argument");
}

int main()
{
    matrix_times_vector();
    encoding_transforms();
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all chained-transform class-layer checks passed\n");
    return 0;
}
