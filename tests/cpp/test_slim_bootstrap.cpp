// Slim, bit and gate bootstrapping through the class layer (include/heongpu/heongpu.hpp: BootstrappingConfig,
// arithmetic_bootstrapping_type, logic_bootstrapping_type, HEArithmeticOperator<CKKS>::generate_bootstrapping_params /
// slim_bootstrapping, HELogicOperator<CKKS>::generate_bootstrapping_params / bootstrapping_key_indexs / bit_bootstrapping /
// AND_bootstrapping / XOR_bootstrapping): the call sequences of the reference's example/bootstrapping/2_..., 3_... and
// 4_... at N = 4096 with secrets of Hamming weight 16, on 18-limb chains:
//   slim   {50, 40 x 5, 50 x 12} | {60}, scale 2^40: 0.2 in every slot -> f(0.2) = (rho / 2 pi) sin(2 pi 0.2 / rho), rho = 256
//   bit    {42, 41 x 17} | {60}, scale 2^41 (q_0 = 2 scale): the example's message, ones with two zeros
//   gates  the first 18 primes of the example's chain (q_0 = 3 * 2^40) | one of its special primes, scale 2^40: AND, XOR
// Every slot within 1e-4, the criterion of this repository's semantic tests.  Checks the exceptions the reference
// throws (the level, the lock, the last modulus, the key indexs before generation), the validation of
// BootstrappingConfig and that REGULAR_BOOTSTRAPPING through the v1 call is refused.  Exits non-zero on a wrong result.
#include <heongpu/heongpu.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace heongpu;
constexpr auto S = Scheme::CKKS;

static int failures = 0;
#define EXPECT(cond, what)                                   \
    do {                                                     \
        if (!(cond)) { failures++; std::printf("FAIL: %s\n", what); } \
        else std::printf("ok:   %s\n", what);                \
    } while (0)

template <typename E, typename F> static bool throws(F&& f, const char* text = nullptr)
{
    try { f(); } catch (const E& e) { return !text || std::strstr(e.what(), text); } catch (...) { return false; }
    return false;
}

static double worst(const std::vector<Complex64>& got, const std::vector<double>& want)
{
    double w = got.size() == want.size() ? 0.0 : 1e9;
    for (size_t i = 0; i < got.size() && i < want.size(); i++)
        w = std::fmax(w, std::hypot(got[i].real() - want[i], got[i].imag()));
    return w;
}

// everything one scenario needs besides its operator
struct Party {
    HEContext<S> ctx;
    HEKeyGenerator<S> keygen;
    Secretkey<S> sk;
    Publickey<S> pk;
    Relinkey<S> rk;
    HEEncoder<S> encoder;
    explicit Party(HEContext<S> c) : ctx(c), keygen(c), sk(c, 16), pk(c), rk(c), encoder(c)
    {
        keygen.generate_secret_key(sk);
        keygen.generate_public_key(pk, sk);
        keygen.generate_relin_key(rk, sk);
    }
    Ciphertext<S> encrypt(const std::vector<double>& message, double scale)
    {
        HEEncryptor<S> enc(ctx, pk);
        Plaintext<S> plain(ctx);
        encoder.encode(plain, message, scale);
        Ciphertext<S> cipher(ctx);
        enc.encrypt(cipher, plain);
        return cipher;
    }
    std::vector<Complex64> decrypt(Ciphertext<S>& cipher)
    {
        HEDecryptor<S> dec(ctx, sk);
        Plaintext<S> p(ctx);
        dec.decrypt(p, cipher);
        std::vector<Complex64> got;
        encoder.decode(got, p);
        return got;
    }
};

static void slim()
{
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({50, 40, 40, 40, 40, 40, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50}, {60});
    ctx->generate();
    const double scale = std::pow(2.0, 40);
    Party party(ctx);
    HEArithmeticOperator<S> op(ctx, party.encoder);
    std::vector<double> message(slots, 0.2); // real numbers: the slim refresh keeps the real parts
    Ciphertext<S> cipher = party.encrypt(message, scale);

    EXPECT(throws<std::out_of_range>([] { BootstrappingConfig(1, 3, 7, true); }) &&
               throws<std::out_of_range>([] { BootstrappingConfig(3, 6, 7, true); }) &&
               throws<std::out_of_range>([] { BootstrappingConfig(3, 3, 16, true); }),
           "BootstrappingConfig validates its pieces and its taylor number (std::out_of_range)");
    BootstrappingConfig defaults;
    EXPECT(defaults.CtoS_piece_ == 3 && defaults.StoC_piece_ == 3 && defaults.taylor_number_ == 11 && !defaults.less_key_mode_,
           "BootstrappingConfig has the reference's defaults");
    const int StoC_piece = 3;
    BootstrappingConfig config(3, StoC_piece, 7, true);
    Galoiskey<S> none(ctx, std::vector<int>{1});
    EXPECT(throws<std::invalid_argument>([&] { op.slim_bootstrapping(cipher, none, party.rk); }),
           "a slim refresh before the parameters are generated is std::invalid_argument");
    EXPECT(throws<std::invalid_argument>(
               [&] { op.generate_bootstrapping_params(scale, config, arithmetic_bootstrapping_type::REGULAR_BOOTSTRAPPING); }),
           "REGULAR_BOOTSTRAPPING through the v1 call is std::invalid_argument (the regular refresh is the v2 call)");
    op.generate_bootstrapping_params(scale, config, arithmetic_bootstrapping_type::SLIM_BOOTSTRAPPING);
    EXPECT(throws<std::runtime_error>(
               [&] { op.generate_bootstrapping_params(scale, config, arithmetic_bootstrapping_type::SLIM_BOOTSTRAPPING); }),
           "the parameters are locked after the first generation (std::runtime_error)");
    BootstrappingConfigV2 v2(EncodingMatrixConfig(LinearTransformType::SLOTS_TO_COEFFS, 5), EvalModConfig(13),
                             EncodingMatrixConfig(LinearTransformType::COEFFS_TO_SLOTS, 17));
    EXPECT(throws<std::runtime_error>([&] { op.generate_bootstrapping_params_v2(scale, v2); }),
           "the one lock holds for the v2 parameters too");
    std::vector<int> key_index = op.bootstrapping_key_indexs();
    std::printf("slim: Galois keys needed: %zu\n", key_index.size());
    EXPECT(!key_index.empty(), "bootstrapping_key_indexs serves the slim parameter set");
    Galoiskey<S> gk(ctx, key_index);
    party.keygen.generate_galois_key(gk, party.sk);

    EXPECT(throws<std::logic_error>([&] { op.slim_bootstrapping(cipher, gk, party.rk); }, "Ciphertexts leveled should be at max!"),
           "a ciphertext that is not at level StoC_piece is std::logic_error");
    for (int i = 0; i < 17 - StoC_piece; i++) op.mod_drop_inplace(cipher);
    Ciphertext<S> fresh = op.slim_bootstrapping(cipher, gk, party.rk);
    std::printf("slim: level after the refresh: %d\n", fresh.level());
    EXPECT(fresh.level() == 5, "the result leaves at the plan's level");
    EXPECT(!fresh.rescale_required() && !fresh.relinearization_required() && fresh.size() == 2,
           "the result is relinearized and rescaled");
    const double rho = 256.0, pi = std::acos(-1.0);
    EXPECT(std::fabs(fresh.scale() * rho / (double) ctx->prime_vector_[13].value - 1.0) <= 1e-12,
           "the result carries the plan's out_scale, the polynomial's scale over rho");
    std::vector<Complex64> got = party.decrypt(fresh);
    const double w = worst(got, std::vector<double>(slots, rho / (2 * pi) * std::sin(2 * pi * 0.2 / rho)));
    std::printf("slim: max |refreshed - f(0.2)| = %.3e over %zu slots (criterion 1e-4)\n", w, got.size());
    EXPECT(w < 1e-4, "every slot holds f(0.2) within 1e-4");
}

static void bit()
{
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({42, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41, 41}, {60});
    ctx->generate();
    const double scale = std::pow(2.0, 41);
    Party party(ctx);
    HELogicOperator<S> op(ctx, party.encoder, scale);
    std::vector<double> message(slots, 1);
    message[0] = 0;
    message[1] = 0;
    Ciphertext<S> cipher = party.encrypt(message, scale);

    const int StoC_piece = 3;
    BootstrappingConfig config(3, StoC_piece, 6, true);
    EXPECT(throws<std::invalid_argument>([&] { op.bootstrapping_key_indexs(); }),
           "bootstrapping_key_indexs before the parameters are generated is std::invalid_argument");
    EXPECT(throws<std::invalid_argument>(
               [&] { op.generate_bootstrapping_params(scale, config, logic_bootstrapping_type::GATE_BOOTSTRAPPING); },
               "Last modulus should be 3*scale!"),
           "gate parameters on a chain whose last modulus is 2 * scale are std::invalid_argument");
    EXPECT(throws<std::invalid_argument>(
               [&] { op.generate_bootstrapping_params(scale / 2, config, logic_bootstrapping_type::BIT_BOOTSTRAPPING); },
               "Last modulus should be 2*scale!"),
           "bit parameters at a scale that is not q_0 / 2 are std::invalid_argument");
    op.generate_bootstrapping_params(scale, config, logic_bootstrapping_type::BIT_BOOTSTRAPPING);
    EXPECT(throws<std::runtime_error>(
               [&] { op.generate_bootstrapping_params(scale, config, logic_bootstrapping_type::BIT_BOOTSTRAPPING); }),
           "the parameters are locked after the first generation (std::runtime_error)");
    std::vector<int> key_index = op.bootstrapping_key_indexs();
    std::printf("bit: Galois keys needed: %zu\n", key_index.size());
    Galoiskey<S> gk(ctx, key_index);
    party.keygen.generate_galois_key(gk, party.sk);
    EXPECT(throws<std::logic_error>([&] { op.bit_bootstrapping(cipher, gk, party.rk); }, "Ciphertexts leveled should be at max!"),
           "a ciphertext that is not at level StoC_piece is std::logic_error");
    for (int i = 0; i < 17 - StoC_piece; i++) op.mod_drop_inplace(cipher);
    EXPECT(throws<std::invalid_argument>([&] { op.AND_bootstrapping(cipher, cipher, gk, party.rk); }),
           "a gate on bit parameters is std::invalid_argument");
    Ciphertext<S> fresh = op.bit_bootstrapping(cipher, gk, party.rk);
    std::printf("bit: level after the refresh: %d\n", fresh.level());
    EXPECT(fresh.level() == 5, "the result leaves at the plan's level");
    std::vector<Complex64> got = party.decrypt(fresh);
    const double w = worst(got, message);
    std::printf("bit: max |refreshed - b| = %.3e over %zu slots (criterion 1e-4)\n", w, got.size());
    EXPECT(w < 1e-4, "every slot holds its bit within 1e-4");
}

static void gates()
{
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_values({3298535538689ULL, 1099512938497ULL, 1099515691009ULL, 1099516870657ULL, 1099521458177ULL,
                                   1099522375681ULL, 1099523555329ULL, 1099525128193ULL, 1099526176769ULL, 1099529060353ULL,
                                   1099535220737ULL, 1099536138241ULL, 1099537580033ULL, 1099538104321ULL, 1099540725761ULL,
                                   1099540856833ULL, 1099543085057ULL, 1099544002561ULL},
                                  {3298535669761ULL});
    ctx->generate();
    const double scale = std::pow(2.0, 40);
    Party party(ctx);
    HELogicOperator<S> op(ctx, party.encoder, scale);
    std::vector<double> message1(slots, 1), message2(slots, 1);
    message1[0] = 0;
    message1[2] = 0;
    message2[2] = 0;
    message2[3] = 0; // (0, 1), (1, 1), (0, 0), (1, 0) in the first four slots
    Ciphertext<S> c1 = party.encrypt(message1, scale), c2 = party.encrypt(message2, scale);

    const int StoC_piece = 3;
    BootstrappingConfig config(3, StoC_piece, 6, true);
    EXPECT(throws<std::invalid_argument>(
               [&] { op.generate_bootstrapping_params(scale, config, logic_bootstrapping_type::BIT_BOOTSTRAPPING); },
               "Last modulus should be 2*scale!"),
           "bit parameters on a chain whose last modulus is 3 * scale are std::invalid_argument");
    op.generate_bootstrapping_params(scale, config, logic_bootstrapping_type::GATE_BOOTSTRAPPING);
    std::vector<int> key_index = op.bootstrapping_key_indexs();
    std::printf("gates: Galois keys needed: %zu\n", key_index.size());
    Galoiskey<S> gk(ctx, key_index);
    party.keygen.generate_galois_key(gk, party.sk);
    for (int i = 0; i < 17 - StoC_piece; i++) {
        op.mod_drop_inplace(c1);
        if (i < 16 - StoC_piece) op.mod_drop_inplace(c2);
    }
    EXPECT(throws<std::logic_error>([&] { op.AND_bootstrapping(c1, c2, gk, party.rk); }, "Ciphertexts leveled should be at max!"),
           "a second input that is not at level StoC_piece is std::logic_error");
    op.mod_drop_inplace(c2);
    EXPECT(throws<std::invalid_argument>([&] { op.bit_bootstrapping(c1, gk, party.rk); }),
           "a bit refresh on gate parameters is std::invalid_argument");
    std::vector<double> want_and(slots), want_xor(slots);
    for (size_t i = 0; i < slots; i++) {
        want_and[i] = (double) (int(message1[i]) & int(message2[i]));
        want_xor[i] = (double) (int(message1[i]) ^ int(message2[i]));
    }
    Ciphertext<S> r_and = op.AND_bootstrapping(c1, c2, gk, party.rk);
    Ciphertext<S> r_xor = op.XOR_bootstrapping(c1, c2, gk, party.rk);
    EXPECT(r_and.level() == 5 && r_xor.level() == 5, "the results leave at the plan's level");
    const double wa = worst(party.decrypt(r_and), want_and), wx = worst(party.decrypt(r_xor), want_xor);
    std::printf("gates: max |refreshed - gate(a, b)|: AND %.3e XOR %.3e over %zu slots (criterion 1e-4)\n", wa, wx, slots);
    EXPECT(wa < 1e-4, "AND_bootstrapping: every slot holds a AND b within 1e-4");
    EXPECT(wx < 1e-4, "XOR_bootstrapping: every slot holds a XOR b within 1e-4");
}

int main()
{
    slim();
    bit();
    gates();
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all slim bootstrap class-layer checks passed\n");
    return 0;
}
