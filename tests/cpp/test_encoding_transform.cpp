// CoeffToSlot / SlotToCoeff through the class layer (include/heongpu/heongpu.hpp: CKKSEncodingTransformConfig,
// CKKSEncodingTransformContext, HEArithmeticOperator::generate_encoding_transform_context / coeff_to_slot /
// slot_to_coeff): generate the context, build the Galois key from key_indexs_, then encrypt a coefficient-encoded
// message -> coeff_to_slot -> slot_to_coeff -> decrypt.  Checks the encodings, the depths (4 after CoeffToSlot from 0
// with three pieces, 8 after SlotToCoeff from 4), the slots after CoeffToSlot (slot j of output 0 = coefficient
// bitrev(j), of output 1 = coefficient N/2 + bitrev(j), |a - b| < 1e-4), the round trip (5e-2) and the exception type
// of every refusal.  Exits non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc encodingtransformtest`.
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

static size_t bitrev(size_t j, int bits)
{
    size_t r = 0;
    for (int b = 0; b < bits; b++) r |= ((j >> b) & 1) << (bits - 1 - b);
    return r;
}

int main()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096, slots = n / 2;
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
    CKKSEncodingTransformContext tc;
    op.generate_encoding_transform_context(tc, scale, config);
    EXPECT(tc.generated_ && tc.CtoS_level_ == 0 && tc.StoC_level_ == 4 && tc.CtoS_piece_ == 3 && tc.StoC_piece_ == 3 &&
               tc.scale_boot_ == scale && !tc.key_indexs_.empty(),
           "the context records its levels, piece counts, scale and rotations");
    Galoiskey<S> gk(ctx, tc.key_indexs_);
    keygen.generate_galois_key(gk, sk);

    std::vector<double> message(n, 0.0);
    const double head[8] = {1.00, -0.50, 0.25, -1.75, 2.50, -3.25, 0.125, -0.875};
    for (int k = 0; k < 8; k++) message[k] = head[k];
    message[slots + 3] = 0.75; // the upper half goes to the second output
    Plaintext<S> plain(ctx);
    encoder.encode(plain, message, scale, ExecutionOptions(), encoding::COEFFICIENT);
    Ciphertext<S> cipher(ctx);
    enc.encrypt(cipher, plain);
    EXPECT(cipher.encoding_type() == encoding::COEFFICIENT, "the input is coefficient-encoded");

    std::vector<Ciphertext<S>> pair = op.coeff_to_slot(cipher, gk, tc);
    EXPECT(pair.size() == 2 && pair[0].encoding_type() == encoding::SLOT && pair[1].encoding_type() == encoding::SLOT,
           "coeff_to_slot returns two slot-encoded ciphertexts");
    EXPECT(pair[0].depth() == 4 && pair[1].depth() == 4, "three pieces from level 0 leave at level 4");
    EXPECT(std::fabs(std::log2(pair[0].scale()) - 40.0) < 0.01 && pair[0].scale() == pair[1].scale(),
           "the scale is tracked through three products and rescales");
    double e_slots = 0;
    for (int r = 0; r < 2; r++) {
        Plaintext<S> p(ctx);
        dec.decrypt(p, pair[r]);
        std::vector<Complex64> got;
        encoder.decode(got, p);
        for (size_t j = 0; j < slots; j++)
            e_slots = std::max(e_slots, std::abs(got[j] - Complex64(message[r * slots + bitrev(j, 11)], 0.0)));
    }
    std::printf("max |slot - coefficient| after coeff_to_slot = %.3e\n", e_slots);
    EXPECT(e_slots < 1e-4, "slot j of output r holds coefficient r N/2 + bitrev(j)");

    Ciphertext<S> back = op.slot_to_coeff(pair[0], pair[1], gk, tc);
    EXPECT(back.encoding_type() == encoding::COEFFICIENT, "slot_to_coeff returns a coefficient-encoded ciphertext");
    EXPECT(back.depth() == 8, "three pieces from level 4 leave at level 8");
    Plaintext<S> p_ref(ctx), p_back(ctx);
    dec.decrypt(p_ref, cipher);
    dec.decrypt(p_back, back);
    std::vector<double> ref, got;
    encoder.decode(ref, p_ref);
    encoder.decode(got, p_back);
    double e_round = 0;
    for (size_t k = 0; k < n; k++) e_round = std::max(e_round, std::fabs(ref[k] - got[k]));
    std::printf("max |round trip - input| = %.3e\n", e_round);
    EXPECT(ref.size() == n && got.size() == n && e_round < 5e-2, "slot_to_coeff(coeff_to_slot(x)) = x");

    // refusals, with the reference's exception types
    {
        CKKSEncodingTransformContext t2;
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {1, 3, 0, 4, false}); }),
               "CtoS_piece outside [2, 5] is std::out_of_range");
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {3, 6, 0, 4, false}); }),
               "StoC_piece outside [2, 5] is std::out_of_range");
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 9, 4, false}); }),
               "CtoS_start_level outside [0, Q - 1] is std::out_of_range");
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 0, 8, false}); }),
               "a StoC_start_level without the extra level is std::out_of_range");
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 7, 4, false}); }),
               "a CtoS_start_level too deep for the pieces is std::out_of_range");
        EXPECT(throws<std::out_of_range>([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 0, 6, false}); }),
               "a StoC_start_level too deep for the pieces is std::out_of_range");
        EXPECT(throws<std::invalid_argument>([&] { op.generate_encoding_transform_context(t2, 0.0, config); }),
               "a zero scale is std::invalid_argument");
        EXPECT(throws<std::invalid_argument>([&] { op.generate_encoding_transform_context(t2, scale, {3, 3, 0, 4, true}); }),
               "less_key_mode is std::invalid_argument");
        EXPECT(!t2.generated_, "a refused generation leaves the context not generated");
        EXPECT(throws<std::invalid_argument>([&] { op.coeff_to_slot(cipher, gk, t2); }),
               "coeff_to_slot with a context that is not generated is std::invalid_argument");
        EXPECT(throws<std::invalid_argument>([&] { op.slot_to_coeff(pair[0], pair[1], gk, t2); }),
               "slot_to_coeff with a context that is not generated is std::invalid_argument");
        EXPECT(throws<std::invalid_argument>([&] { op.coeff_to_slot(pair[0], gk, tc); }),
               "coeff_to_slot of a slot-encoded ciphertext is std::invalid_argument");
        EXPECT(throws<std::invalid_argument>([&] { op.slot_to_coeff(cipher, pair[1], gk, tc); }),
               "slot_to_coeff of a coefficient-encoded ciphertext is std::invalid_argument");
        Ciphertext<S> dropped(ctx);
        op.mod_drop(cipher, dropped);
        dropped.encoding_ = encoding::COEFFICIENT;
        EXPECT(throws<std::logic_error>([&] { op.coeff_to_slot(dropped, gk, tc); }),
               "coeff_to_slot at another level than CtoS_start_level is std::logic_error");
        Ciphertext<S> deeper(ctx);
        op.mod_drop(pair[1], deeper);
        deeper.encoding_ = encoding::SLOT;
        EXPECT(throws<std::logic_error>([&] { op.slot_to_coeff(pair[0], deeper, gk, tc); }),
               "slot_to_coeff of two levels is std::logic_error");
        EXPECT(throws<std::logic_error>([&] { op.slot_to_coeff(deeper, deeper, gk, tc); }),
               "slot_to_coeff at another level than StoC_start_level is std::logic_error");
        Galoiskey<S> few(ctx, std::vector<int>{1, 2});
        keygen.generate_galois_key(few, sk);
        EXPECT(throws<std::invalid_argument>([&] { op.coeff_to_slot(cipher, few, tc); }),
               "a rotation without its own key is std::invalid_argument");
    }

    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("all encoding-transform class-layer checks passed\n");
    return 0;
}
