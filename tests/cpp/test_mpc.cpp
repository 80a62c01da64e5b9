// Three parties through the multiparty class layer (include/heongpu/heongpu.hpp: RNGSeed, Multiparty*key,
// HEMultiPartyManager): collective keys -> encrypt -> multiply -> relinearize -> rotate -> decrypt_partial x 3 ->
// decrypt, for CKKS and BFV.  Exits non-zero on a wrong result.  Built by `make -C heongpu_amd/csrc mpctest`.
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

template <typename F> static bool throws_invalid(F&& f)
{
    try { f(); } catch (const std::invalid_argument&) { return true; } catch (...) { return false; }
    return false;
}
template <typename F> static bool throws_logic(F&& f)
{
    try { f(); } catch (const std::logic_error&) { return true; } catch (...) { return false; }
    return false;
}

// the collective keys of `parties` managers, the way a server assembles them
template <Scheme S> struct Collective {
    Publickey<S> pk;
    Relinkey<S> rk;
    Galoiskey<S> gk;
};

template <Scheme S>
static void collective_keys(HEContext<S> ctx, std::vector<HEMultiPartyManager<S>*>& mgr, std::vector<Secretkey<S>>& sk,
                            HEMultiPartyManager<S>& server, const RNGSeed& seed, std::vector<int>& shifts, Collective<S>& out)
{
    const size_t k = mgr.size();
    std::vector<MultipartyPublickey<S>> pks;
    std::vector<MultipartyRelinkey<S>> rk1, rk2;
    std::vector<MultipartyGaloiskey<S>> gks;
    for (size_t i = 0; i < k; i++) {
        MultipartyPublickey<S> pk(ctx, seed);
        mgr[i]->generate_public_key_share(pk, sk[i]);
        pks.push_back(pk);
        MultipartyRelinkey<S> r(ctx, seed);
        mgr[i]->generate_relin_key_init(r, sk[i]);
        rk1.push_back(r);
        MultipartyGaloiskey<S> g(ctx, shifts, seed);
        mgr[i]->generate_galois_key_share(g, sk[i]);
        gks.push_back(g);
    }
    EXPECT(throws_logic([&] { mgr[0]->generate_public_key_share(pks[0], sk[0]); }), "Publickey is already generated");
    server.assemble_public_key_share(pks, out.pk);
    MultipartyRelinkey<S> common1(ctx, seed);
    server.assemble_relin_key_init(rk1, common1);
    server.assemble_galois_key_share(gks, out.gk);
    for (size_t i = 0; i < k; i++) {
        MultipartyRelinkey<S> r(ctx, seed);
        mgr[i]->generate_relin_key_share(common1, r, sk[i]);
        rk2.push_back(r);
    }
    server.assemble_relin_key_share(rk2, common1, out.rk);
    std::vector<MultipartyPublickey<S>> none;
    EXPECT(throws_invalid([&] { Publickey<S> p(ctx); server.assemble_public_key_share(none, p); }),
           "No participant to generate common publickey");
}

template <Scheme S>
static void open(std::vector<HEMultiPartyManager<S>*>& mgr, std::vector<Secretkey<S>>& sk, Ciphertext<S>& ct, HEContext<S> ctx,
                 Plaintext<S>& out)
{
    std::vector<Ciphertext<S>> partial;
    for (size_t i = 0; i < mgr.size(); i++) {
        Ciphertext<S> p(ctx);
        mgr[i]->decrypt_partial(ct, sk[i], p);
        partial.push_back(p);
    }
    mgr[0]->decrypt(partial, out);
}

static void ckks()
{
    constexpr auto S = Scheme::CKKS;
    const size_t n = 4096, slots = n / 2;
    HEContext<S> ctx = GenHEContext<S>(sec_level_type::none);
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_bit_sizes({50, 30, 30, 30}, {50});
    ctx->generate();
    double scale = std::pow(2.0, 30);
    HEEncoder<S> encoder(ctx);
    RNGSeed seed;
    std::vector<int> shifts{1};
    HEMultiPartyManager<S> alice(ctx, encoder, scale), bob(ctx, encoder, scale), charlie(ctx, encoder, scale),
        server(ctx, encoder, scale);
    std::vector<HEMultiPartyManager<S>*> mgr{&alice, &bob, &charlie};
    std::vector<Secretkey<S>> sk;
    for (int i = 0; i < 3; i++) {
        HEKeyGenerator<S> keygen(ctx);
        Secretkey<S> s(ctx);
        keygen.generate_secret_key(s);
        sk.push_back(s);
    }
    Collective<S> keys{Publickey<S>(ctx), Relinkey<S>(ctx), Galoiskey<S>(ctx, shifts)};
    collective_keys<S>(ctx, mgr, sk, server, seed, shifts, keys);

    std::vector<double> a(slots), b(slots), got;
    for (size_t i = 0; i < slots; i++) { a[i] = 1.0 + 0.001 * (double) (i % 97); b[i] = 2.0 - 0.002 * (double) (i % 89); }
    HEEncryptor<S> enc(ctx, keys.pk);
    HEArithmeticOperator<S> op(ctx);
    Plaintext<S> pa(ctx), pb(ctx), out(ctx);
    encoder.encode(pa, a, scale);
    encoder.encode(pb, b, scale);
    Ciphertext<S> ca(ctx), cb(ctx), prod(ctx), rot(ctx);
    enc.encrypt(ca, pa);
    enc.encrypt(cb, pb);
    open<S>(mgr, sk, ca, ctx, out);
    encoder.decode(got, out);
    double err = 0;
    for (size_t i = 0; i < slots; i++) err = std::max(err, std::fabs(got[i] - a[i]));
    EXPECT(got.size() == slots && err < 1e-4, "ckks: collective decryption of a fresh ciphertext");
    op.multiply(ca, cb, prod);
    EXPECT(throws_invalid([&] { Ciphertext<S> p(ctx); alice.decrypt_partial(prod, sk[0], p); }),
           "ckks: a 3-part ciphertext must be relinearized before decrypt_partial");
    op.relinearize_inplace(prod, keys.rk);
    op.rescale_inplace(prod);
    op.rotate_rows(prod, rot, keys.gk, 1);
    open<S>(mgr, sk, rot, ctx, out);
    encoder.decode(got, out);
    err = 0;
    for (size_t i = 0; i < slots; i++) err = std::max(err, std::fabs(got[i] - a[(i + 1) % slots] * b[(i + 1) % slots]));
    std::printf("ckks: max slot error after multiply, relinearize, rescale, rotate = %g\n", err);
    EXPECT(err < 1e-3, "ckks: rotate(relinearize(a * b)) under collective keys, opened by three partial decryptions");
    std::vector<Ciphertext<S>> none;
    EXPECT(throws_invalid([&] { alice.decrypt(none, out); }), "ckks: No ciphertext to decrypt");
}

static void bfv()
{
    constexpr auto S = Scheme::BFV;
    const size_t n = 4096;
    const Data64 t = 1032193;
    HEContext<S> ctx = GenHEContext<S>();
    ctx->set_poly_modulus_degree(n);
    ctx->set_coeff_modulus_default_values(1);
    ctx->set_plain_modulus(t);
    ctx->generate();
    HEEncoder<S> encoder(ctx);
    RNGSeed seed;
    std::vector<int> shifts{1};
    HEMultiPartyManager<S> alice(ctx), bob(ctx), charlie(ctx), server(ctx);
    std::vector<HEMultiPartyManager<S>*> mgr{&alice, &bob, &charlie};
    std::vector<Secretkey<S>> sk;
    for (int i = 0; i < 3; i++) {
        HEKeyGenerator<S> keygen(ctx);
        Secretkey<S> s(ctx);
        keygen.generate_secret_key(s);
        sk.push_back(s);
    }
    Collective<S> keys{Publickey<S>(ctx), Relinkey<S>(ctx), Galoiskey<S>(ctx, shifts)};
    collective_keys<S>(ctx, mgr, sk, server, seed, shifts, keys);

    std::vector<uint64_t> a(n), b(n), got;
    for (size_t i = 0; i < n; i++) { a[i] = (i * 7 + 1) % t; b[i] = (i * i + 3) % t; }
    HEEncryptor<S> enc(ctx, keys.pk);
    HEArithmeticOperator<S> op(ctx);
    Plaintext<S> pa(ctx), pb(ctx), out(ctx);
    encoder.encode(pa, a);
    encoder.encode(pb, b);
    Ciphertext<S> ca(ctx), cb(ctx), rot(ctx);
    enc.encrypt(ca, pa);
    enc.encrypt(cb, pb);
    op.multiply_inplace(ca, cb);
    op.relinearize_inplace(ca, keys.rk);
    op.rotate_rows(ca, rot, keys.gk, 1);
    open<S>(mgr, sk, rot, ctx, out);
    encoder.decode(got, out);
    bool ok = got.size() == n;
    for (size_t i = 0; ok && i < n / 2; i++) {
        const size_t j = (i + 1) % (n / 2);
        ok = got[i] == (a[j] * b[j]) % t && got[n / 2 + i] == (a[n / 2 + j] * b[n / 2 + j]) % t;
    }
    EXPECT(ok, "bfv: rotate(relinearize(a * b)) under collective keys, opened by three partial decryptions, exact");
}

int main()
{
    ckks();
    bfv();
    std::printf(failures ? "%d check(s) failed\n" : "all multiparty class-layer checks passed\n", failures);
    return failures ? 1 : 0;
}
