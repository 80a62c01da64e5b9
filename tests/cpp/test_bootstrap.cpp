// The CKKS refresh through the class layer (include/heongpu/heongpu.hpp: EvalModConfig, EncodingMatrixConfig,
// BootstrappingConfigV2, HEArithmeticOperator<CKKS>::generate_bootstrapping_params_v2, bootstrapping_key_indexs,
// regular_bootstrapping_v2, HEKeyGenerator::generate_secret_key_v2, PrecisionStats): the call sequence of the reference's
// example/bootstrapping/5_ckks_regular_bootstrapping_v2.cpp at N = 4096 on the 18-limb chain
// {50, 40 x 5, 50 x 12} | {60} of tests/test_gpu_bootstrap.py -- a dense secret, an ephemeral sparse one of weight 32 and
// both switch keys, 0.2 + 0.4 i in every slot at scale 2^40, every level dropped but one, refreshed, decrypted, decoded.
// The refresh acts on the coefficients, a -> f(a) = (rho / 2 pi) sin(2 pi a / rho), rho = q_0 / (k1 scale) = 256 here, and
// the constant slot vector has the coefficients 0.2 (index 0) and 0.4 (index N / 2): every slot must hold
// f(0.2) + f(0.4) i, within the 1e-4 of this repository's semantic tests (tests/test_gpu_bootstrap.py measures 5e-6).
// Checks the two exceptions of regular_bootstrapping_v2 and that the parameters lock.  Exits non-zero on a wrong result.
#include <heongpu/heongpu.hpp>

#include <cmath>
#include <cstdio>
#include <iostream>
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

int main()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({50, 40, 40, 40, 40, 40, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50}, {60});
    ctx->generate();
    const double scale = std::pow(2.0, 40);

    HEKeyGenerator<S> keygen(ctx);
    Secretkey<S> sk(ctx, 192);
    keygen.generate_secret_key_v2(sk);
    Publickey<S> pk(ctx);
    keygen.generate_public_key(pk, sk);
    Relinkey<S> rk(ctx);
    keygen.generate_relin_key(rk, sk);
    Secretkey<S> sparse(ctx, 32);
    keygen.generate_secret_key_v2(sparse);
    Switchkey<S> down(ctx), up(ctx);
    keygen.generate_switch_key(down, sparse, sk); // dense -> sparse
    keygen.generate_switch_key(up, sk, sparse);   // sparse -> dense

    HEEncoder<S> encoder(ctx);
    HEEncryptor<S> enc(ctx, pk);
    HEDecryptor<S> dec(ctx, sk);
    HEArithmeticOperator<S> op(ctx, encoder);

    std::vector<Complex64> message(slots, Complex64(0.2, 0.4));
    Plaintext<S> plain(ctx);
    encoder.encode(plain, message, scale);
    Ciphertext<S> cipher(ctx);
    enc.encrypt(cipher, plain);

    Galoiskey<S> none(ctx, std::vector<int>{1});
    EXPECT(throws<std::invalid_argument>([&] { op.regular_bootstrapping_v2(cipher, none, rk, &down, &up); }),
           "a refresh before the parameters are generated is std::invalid_argument");

    EvalModConfig eval_mod(13);
    EXPECT(eval_mod.K_ == 16 && eval_mod.sine_deg_ == 30 && eval_mod.double_angle_ == 3 && eval_mod.message_ratio_ == 256.0,
           "EvalModConfig(level_start) has the reference's defaults");
    eval_mod.K_ = 12;
    BootstrappingConfigV2 config(EncodingMatrixConfig(LinearTransformType::SLOTS_TO_COEFFS, 5), eval_mod,
                                 EncodingMatrixConfig(LinearTransformType::COEFFS_TO_SLOTS, 17));
    EXPECT(config.CtoS_piece_ == 4 && config.StoC_piece_ == 3, "EncodingMatrixConfig has the reference's default piece counts");
    op.generate_bootstrapping_params_v2(scale, config);
    EXPECT(throws<std::runtime_error>([&] { op.generate_bootstrapping_params_v2(scale, config); }),
           "the parameters are locked after the first generation (std::runtime_error)");

    std::vector<int> key_index = op.bootstrapping_key_indexs();
    std::printf("Galois keys needed: %zu\n", key_index.size());
    EXPECT(!key_index.empty(), "bootstrapping_key_indexs lists the rotations of the factors");
    Galoiskey<S> gk(ctx, key_index);
    keygen.generate_galois_key(gk, sk);

    EXPECT(throws<std::logic_error>([&] { op.regular_bootstrapping_v2(cipher, gk, rk, &down, &up); }),
           "a ciphertext that is not at its last level is std::logic_error");
    for (int i = 0; i < 17; i++) op.mod_drop_inplace(cipher);
    EXPECT(cipher.level() == 0, "every level dropped but one");
    EXPECT(throws<std::invalid_argument>([&] { op.regular_bootstrapping_v2(cipher, gk, rk, &down, nullptr); }),
           "one switch key without the other is std::invalid_argument");

    Ciphertext<S> fresh = op.regular_bootstrapping_v2(cipher, gk, rk, &down, &up);
    std::printf("level after the refresh: %d\n", fresh.level());
    EXPECT(fresh.level() == 1, "the result leaves at the plan's level");
    EXPECT(std::fabs(fresh.scale() / scale - 1.0) <= 1e-12, "the result carries the caller's scale");
    EXPECT(!fresh.rescale_required() && !fresh.relinearization_required() && fresh.size() == 2,
           "the result is relinearized and rescaled");
    Plaintext<S> p(ctx);
    dec.decrypt(p, fresh);
    std::vector<Complex64> got;
    encoder.decode(got, p);
    const double rho = (double) ctx->prime_vector_[0].value / (4.0 * scale), pi = std::acos(-1.0);
    auto f = [&](double a) { return rho / (2 * pi) * std::sin(2 * pi * a / rho); };
    std::vector<Complex64> want(slots, Complex64(f(0.2), f(0.4)));
    PrecisionStats stats = get_precision_stats(want, got);
    std::cout << stats.to_string();
    std::printf("max |refreshed - (f(0.2) + f(0.4) i)|: real %.3e imag %.3e (criterion 1e-4)\n", stats.max_delta.real,
                stats.max_delta.imag);
    EXPECT(got.size() == slots && stats.max_delta.real < 1e-4 && stats.max_delta.imag < 1e-4,
           "every slot holds f(0.2) + f(0.4) i within 1e-4");
    EXPECT(stats.min_precision.l2 > 13.0 && stats.mean_precision.l2 >= stats.min_precision.l2,
           "PrecisionStats reports the bits behind that distance");

    // without switch keys the raise happens under the caller's own (dense) secret: the overflow leaves K, the call is valid
    // and the values are not -- only that it runs is checked
    Ciphertext<S> direct = op.regular_bootstrapping_v2(cipher, gk, rk);
    EXPECT(direct.level() == 1, "the switch keys are optional");

    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all bootstrap class-layer checks passed\n");
    return 0;
}
