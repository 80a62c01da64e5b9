// A plaintext matrix times an encrypted vector through the class layer (include/heongpu/heongpu.hpp: LinearTransform,
// HEArithmeticOperator::linear_transform): build the transform from its diagonals, the Galois key from
// required_shifts(), then encrypt -> linear_transform -> rescale_inplace -> decrypt -> decode against the dense
// product, under the reference tests' criterion |a - b| < 1e-4 (test/test_ckks_relinearization.cpp:9-34).  Exits
// non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc lineartransformtest`.
#include <heongpu/heongpu.hpp>

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

int main()
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

    // real diagonals and a real vector
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

    LinearTransform<S> lt(ctx, diag, encoder, scale);
    EXPECT(lt.n1() == 4 && lt.n2() == 7 && lt.diagonal_count() == 10, "ten diagonals: period 4, 4 baby and 7 giant steps");
    const std::vector<int> shifts = lt.required_shifts();
    EXPECT(shifts.size() == 9, "required_shifts: 1, 2, 3 and the six non-zero giant steps");

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
    double e = 0;
    for (int s = 0; s < slots; s++) e = std::max(e, std::fabs(got[s] - want[s]));
    std::printf("max |decode - M v| = %.3e\n", e);
    EXPECT(e < 1e-4, "decode(decrypt(rescale(linear_transform(enc(v))))) = M v");

    // complex diagonals, a chosen period, one level down
    {
        std::map<int, std::vector<Complex64>> cd;
        for (int k : {0, 7, -1}) {
            std::vector<Complex64> d(slots);
            for (Complex64& x : d) x = Complex64(unit(gen), unit(gen));
            cd[k] = d;
        }
        LinearTransform<S> lc(ctx, cd, encoder, scale, 1, 8);
        Galoiskey<S> gc(ctx, lc.required_shifts());
        keygen.generate_galois_key(gc, sk);
        Ciphertext<S> c1(ctx), c2(ctx);
        op.mod_drop(cv, c1);
        op.linear_transform(c1, lc, gc, c2);
        op.rescale_inplace(c2);
        dec.decrypt(pr, c2);
        std::vector<Complex64> gotc;
        encoder.decode(gotc, pr);
        double ec = 0;
        for (int s = 0; s < slots; s++) {
            Complex64 w(0, 0);
            for (const auto& d : cd) w += d.second[s] * v[((s + d.first) % slots + slots) % slots];
            ec = std::max(ec, std::abs(gotc[s] - w));
        }
        std::printf("max |decode - M v| (complex, depth 1) = %.3e\n", ec);
        EXPECT(ec < 1e-4, "complex diagonals at depth 1 with a chosen period");
        EXPECT(throws_invalid([&] { op.linear_transform(cv, lc, gc, c2); }), "a depth mismatch is std::invalid_argument");
    }

    // refusals
    {
        Galoiskey<S> few(ctx, std::vector<int>{1, 2, 4, 8});
        keygen.generate_galois_key(few, sk);
        Ciphertext<S> out(ctx);
        EXPECT(throws_invalid([&] { op.linear_transform(cv, lt, few, out); }),
               "a shift without its own key is std::invalid_argument (no power-of-two chain)");
        Ciphertext<S> sq(ctx);
        op.multiply(cv, cv, sq);
        EXPECT(throws_invalid([&] { op.linear_transform(sq, lt, gk, out); }), "a 3-part input is std::invalid_argument");
        Ciphertext<S> pending(ctx);
        op.linear_transform(cv, lt, gk, pending);
        EXPECT(throws_invalid([&] { op.linear_transform(pending, lt, gk, out); }),
               "an input awaiting its rescale is std::invalid_argument");
        std::map<int, std::vector<double>> many;
        for (int k = 0; k < 17; k++) many[k * 16] = std::vector<double>(slots, 1.0);
        EXPECT(throws_invalid([&] { LinearTransform<S> big(ctx, many, encoder, scale, 0, 16); }),
               "a plan of more than 16 giant steps is refused");
    }

    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all linear-transform class-layer checks passed\n");
    return 0;
}
