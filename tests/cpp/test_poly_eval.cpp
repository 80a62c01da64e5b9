// A polynomial evaluated on a ciphertext through the class layer (include/heongpu/heongpu.hpp: PolyType, Polynomial,
// HEArithmeticOperator<CKKS>::evaluate_poly): encrypt 2048 values of [-1, 1] at scale 2^40 on a [60, 40 x 7 | 60] chain,
// evaluate the degree-31 Chebyshev interpolant of 1 / (1 + exp(-4x)) and a degree-7 monomial polynomial, decrypt, decode
// and compare with the polynomial in double.  The criterion is the one of
// tests/test_gpu_poly_eval.py::test_poly_eval_semantics: within 8 x the error of the step-by-step composition of single
// entries on such inputs, measured there (1.771e-08 for the Chebyshev case, 2.116e-08 for the monomial one; the factor covers
// the spread of encryption noise across seeds).  Checks the result's depth_, scale_ and flags and the exception type of
// every refusal.  Exits non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc polyevaltest`.
#include <heongpu/heongpu.hpp>

#include <cmath>
#include <cstdio>
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

// RECORDED figures, not measured here: the composition's error as tests/test_gpu_poly_eval.py::test_poly_eval_semantics
// printed it on an MI355X (same chain, scale and polynomials; another message and other keys, which the factor 8 covers).
// That test measures its bound anew on every run; this one does not follow a change in noise behaviour until the two
// numbers are recorded again.
static const double kCompositionError[2] = {1.771e-08, 2.116e-08};

static double sigmoid(double x) { return 1.0 / (1.0 + std::exp(-4.0 * x)); }

static double chebval(const std::vector<Complex64>& c, double x)
{
    double b1 = 0, b2 = 0; // Clenshaw
    for (size_t k = c.size() - 1; k >= 1; k--) {
        const double b0 = c[k].real() + 2 * x * b1 - b2;
        b2 = b1;
        b1 = b0;
    }
    return c[0].real() + x * b1 - b2;
}

int main()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({60, 40, 40, 40, 40, 40, 40, 40}, {60});
    ctx->generate();
    const double scale = std::pow(2.0, 40);

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
    HEArithmeticOperator<S> op(ctx, encoder);

    std::vector<double> message(slots);
    for (size_t j = 0; j < slots; j++) message[j] = -1.0 + 2.0 * (double) ((j * 2654435761u) % 100003) / 100002.0;
    Plaintext<S> plain(ctx);
    encoder.encode(plain, message, scale);
    Ciphertext<S> cipher(ctx);
    enc.encrypt(cipher, plain);

    // degree-31 Chebyshev interpolant at the 32 Chebyshev nodes
    const int M = 32;
    const double pi = std::acos(-1.0);
    std::vector<Complex64> cheb(M);
    for (int k = 0; k < M; k++) {
        double s = 0;
        for (int j = 0; j < M; j++) {
            const double th = (j + 0.5) * pi / M;
            s += sigmoid(std::cos(th)) * std::cos(k * th);
        }
        cheb[k] = Complex64((k ? 2.0 : 1.0) * s / M, 0.0);
    }
    const std::vector<Complex64> mono = {0.5, -0.25, 0.125, 0.75, -0.5, 0.3, -0.2, 0.1};
    const Polynomial polys[2] = {Polynomial(31, cheb, true, PolyType::CHEBYSHEV, -1.0, 1.0),
                                 Polynomial(7, mono, true, PolyType::MONOMIAL)};
    EXPECT(polys[0].degree() == 31 && polys[0].depth() == 5 && polys[1].degree() == 7 && polys[1].depth() == 3,
           "Polynomial reports its degree and depth");

    for (int which = 0; which < 2; which++) {
        Ciphertext<S> res = op.evaluate_poly(cipher, scale, polys[which], rk);
        EXPECT(!res.rescale_required() && !res.relinearization_required() && res.size() == 2,
               "the result is relinearized and rescaled");
        EXPECT(res.depth() == (which == 0 ? 5 : 3), "the result carries the plan's depth");
        EXPECT(std::fabs(std::log2(res.scale()) - 40.0) < 1e-3, "the result carries the plan's scale");
        Plaintext<S> p(ctx);
        dec.decrypt(p, res);
        std::vector<double> got;
        encoder.decode(got, p);
        double e = 0;
        for (size_t j = 0; j < slots; j++) {
            double want;
            if (which == 0) want = chebval(cheb, message[j]);
            else {
                want = 0;
                for (size_t k = mono.size(); k-- > 0;) want = want * message[j] + mono[k].real();
            }
            e = std::max(e, std::fabs(got[j] - want));
        }
        std::printf("polynomial %d: max |decrypted - polynomial| = %.3e, bound %.3e\n", which, e, 8 * kCompositionError[which]);
        EXPECT(e <= 8 * kCompositionError[which], "evaluate_poly computes the polynomial within 8 x the composition's error");
    }

    // refusals, in the reference's style
    {
        Ciphertext<S> prod(ctx);
        op.multiply(cipher, cipher, prod);
        EXPECT(throws<std::invalid_argument>([&] { op.evaluate_poly(prod, scale, polys[1], rk); }),
               "a ciphertext of three parts is std::invalid_argument");
        op.relinearize_inplace(prod, rk);
        EXPECT(throws<std::invalid_argument>([&] { op.evaluate_poly(prod, scale, polys[1], rk); }),
               "a ciphertext that still needs its rescale is std::invalid_argument");
        Ciphertext<S> low(ctx), tmp(ctx);
        op.mod_drop(cipher, low);
        for (int k = 0; k < 4; k++) { op.mod_drop(low, tmp); low = tmp; }
        EXPECT(throws<std::invalid_argument>([&] { op.evaluate_poly(low, scale, polys[0], rk); }),
               "too few levels for the polynomial's depth is std::invalid_argument");
        HEContext<S> other = GenHEContext<S>(sec_level_type::none);
        other->set_poly_modulus_degree(n);
        other->set_coeff_modulus_bit_sizes({60, 40, 40, 40}, {60});
        other->generate();
        HEKeyGenerator<S> keygen2(other);
        Secretkey<S> sk2(other);
        keygen2.generate_secret_key(sk2);
        Relinkey<S> rk2(other);
        keygen2.generate_relin_key(rk2, sk2);
        EXPECT(throws<std::invalid_argument>([&] { op.evaluate_poly(cipher, scale, polys[1], rk2); }),
               "a relinearization key of another context is std::invalid_argument");
        // (a CKKS ciphertext outside the NTT domain cannot be made through the class layer; that check has no case here)
        EXPECT(throws<std::invalid_argument>([&] { op.evaluate_poly(cipher, scale, Polynomial(1, {1.0, 2.0}, true), rk); }),
               "a polynomial of degree 1 is std::invalid_argument");
    }

    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all poly-eval class-layer checks passed\n");
    return 0;
}
