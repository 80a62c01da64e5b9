// Three parties refresh an exhausted ciphertext through the multiparty class layer (include/heongpu/heongpu.hpp:
// HEMultiPartyManager::distributed_bootstrapping_participant / _coordinator): collective keys -> encrypt -> multiply ->
// mod-drop to the last level (CKKS) -> refresh -> multiply again -> collective decryption, for CKKS and BFV.  Exits
// non-zero on a wrong result.  Compiled and run by tests/test_mpc_refresh_class_layer.py.
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

template <Scheme S> struct Party {
    std::vector<HEMultiPartyManager<S>*> mgr;
    std::vector<Secretkey<S>> sk;
};

// public and relinearisation key under the sum of the parties' secrets
template <Scheme S>
static void collective_keys(HEContext<S> ctx, Party<S>& p, HEMultiPartyManager<S>& server, const RNGSeed& seed, Publickey<S>& pk,
                            Relinkey<S>& rk)
{
    std::vector<MultipartyPublickey<S>> pks;
    std::vector<MultipartyRelinkey<S>> rk1, rk2;
    for (size_t i = 0; i < p.mgr.size(); i++) {
        MultipartyPublickey<S> share(ctx, seed);
        p.mgr[i]->generate_public_key_share(share, p.sk[i]);
        pks.push_back(share);
        MultipartyRelinkey<S> r(ctx, seed);
        p.mgr[i]->generate_relin_key_init(r, p.sk[i]);
        rk1.push_back(r);
    }
    server.assemble_public_key_share(pks, pk);
    MultipartyRelinkey<S> common1(ctx, seed);
    server.assemble_relin_key_init(rk1, common1);
    for (size_t i = 0; i < p.mgr.size(); i++) {
        MultipartyRelinkey<S> r(ctx, seed);
        p.mgr[i]->generate_relin_key_share(common1, r, p.sk[i]);
        rk2.push_back(r);
    }
    server.assemble_relin_key_share(rk2, common1, rk);
}

template <Scheme S> static void refresh(HEContext<S> ctx, Party<S>& p, HEMultiPartyManager<S>& server, Ciphertext<S>& ct, Ciphertext<S>& out)
{
    RNGSeed seed; // agreed for this refresh
    std::vector<Ciphertext<S>> shares;
    for (size_t i = 0; i < p.mgr.size(); i++) {
        Ciphertext<S> h(ctx);
        p.mgr[i]->distributed_bootstrapping_participant(ct, h, p.sk[i], seed);
        shares.push_back(h);
    }
    server.distributed_bootstrapping_coordinator(shares, ct, out, seed);
}

template <Scheme S> static void open(HEContext<S> ctx, Party<S>& p, Ciphertext<S>& ct, Plaintext<S>& out)
{
    std::vector<Ciphertext<S>> partial;
    for (size_t i = 0; i < p.mgr.size(); i++) {
        Ciphertext<S> h(ctx);
        p.mgr[i]->decrypt_partial(ct, p.sk[i], h);
        partial.push_back(h);
    }
    p.mgr[0]->decrypt(partial, out);
}

template <Scheme S> static void make_secrets(HEContext<S> ctx, Party<S>& p)
{
    for (size_t i = 0; i < p.mgr.size(); i++) {
        HEKeyGenerator<S> keygen(ctx);
        Secretkey<S> s(ctx);
        keygen.generate_secret_key(s);
        p.sk.push_back(s);
    }
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
    HEMultiPartyManager<S> alice(ctx, encoder, scale), bob(ctx, encoder, scale), charlie(ctx, encoder, scale),
        server(ctx, encoder, scale);
    Party<S> p{{&alice, &bob, &charlie}, {}};
    make_secrets<S>(ctx, p);
    Publickey<S> pk(ctx);
    Relinkey<S> rk(ctx);
    collective_keys<S>(ctx, p, server, RNGSeed(), pk, rk);

    std::vector<double> a(slots), b(slots), got;
    for (size_t i = 0; i < slots; i++) { a[i] = 1.0 + 0.001 * (double) (i % 97); b[i] = 1.5 - 0.002 * (double) (i % 89); }
    HEEncryptor<S> enc(ctx, pk);
    HEArithmeticOperator<S> op(ctx);
    Plaintext<S> pa(ctx), pb(ctx), out(ctx);
    encoder.encode(pa, a, scale);
    encoder.encode(pb, b, scale);
    Ciphertext<S> ca(ctx), cb(ctx), prod(ctx), fresh(ctx), again(ctx);
    enc.encrypt(ca, pa);
    enc.encrypt(cb, pb);
    op.multiply(ca, cb, prod);
    EXPECT(throws_invalid([&] { Ciphertext<S> h(ctx); alice.distributed_bootstrapping_participant(prod, h, p.sk[0], RNGSeed()); }),
           "ckks: a 3-part ciphertext is refused");
    op.relinearize_inplace(prod, rk);
    EXPECT(throws_invalid([&] { Ciphertext<S> h(ctx); alice.distributed_bootstrapping_participant(prod, h, p.sk[0], RNGSeed()); }),
           "ckks: a ciphertext that awaits its rescale is refused");
    op.rescale_inplace(prod);
    while (prod.depth() < 3) op.mod_drop_inplace(prod); // the last level: nothing left to rescale by
    const double scale_in = prod.scale();
    refresh<S>(ctx, p, server, prod, fresh);
    EXPECT(fresh.depth() == 0 && fresh.size() == 2 && fresh.scale() == scale_in, "ckks: the result is at depth 0 with the input's scale");
    open<S>(ctx, p, fresh, out);
    encoder.decode(got, out);
    double err = 0;
    for (size_t i = 0; i < slots; i++) err = std::max(err, std::fabs(got[i] - a[i] * b[i]));
    std::printf("ckks: max slot error after the refresh = %g\n", err);
    EXPECT(got.size() == slots && err < 1e-3, "ckks: the refreshed ciphertext decrypts to a * b");
    op.multiply(fresh, cb, again);
    op.relinearize_inplace(again, rk);
    op.rescale_inplace(again);
    open<S>(ctx, p, again, out);
    encoder.decode(got, out);
    err = 0;
    for (size_t i = 0; i < slots; i++) err = std::max(err, std::fabs(got[i] - a[i] * b[i] * b[i]));
    std::printf("ckks: max slot error after refresh, multiply, relinearize, rescale = %g\n", err);
    EXPECT(err < 1e-2, "ckks: the refreshed ciphertext multiplies again");
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
    HEMultiPartyManager<S> alice(ctx), bob(ctx), charlie(ctx), server(ctx);
    Party<S> p{{&alice, &bob, &charlie}, {}};
    make_secrets<S>(ctx, p);
    Publickey<S> pk(ctx);
    Relinkey<S> rk(ctx);
    collective_keys<S>(ctx, p, server, RNGSeed(), pk, rk);

    std::vector<uint64_t> a(n), b(n), got;
    for (size_t i = 0; i < n; i++) { a[i] = (i * 7 + 1) % t; b[i] = (i * i + 3) % t; }
    HEEncryptor<S> enc(ctx, pk);
    HEArithmeticOperator<S> op(ctx);
    Plaintext<S> pa(ctx), pb(ctx), out(ctx);
    encoder.encode(pa, a);
    encoder.encode(pb, b);
    Ciphertext<S> ca(ctx), cb(ctx), fresh(ctx);
    enc.encrypt(ca, pa);
    enc.encrypt(cb, pb);
    op.multiply_inplace(ca, cb);
    EXPECT(throws_invalid([&] { Ciphertext<S> h(ctx); alice.distributed_bootstrapping_participant(ca, h, p.sk[0], RNGSeed()); }),
           "bfv: a 3-part ciphertext is refused");
    op.relinearize_inplace(ca, rk);
    refresh<S>(ctx, p, server, ca, fresh);
    op.multiply_inplace(fresh, cb);
    op.relinearize_inplace(fresh, rk);
    open<S>(ctx, p, fresh, out);
    encoder.decode(got, out);
    bool ok = got.size() == n;
    for (size_t i = 0; ok && i < n; i++) ok = got[i] == (a[i] * b[i] % t) * b[i] % t;
    EXPECT(ok, "bfv: refresh(a * b) * b under collective keys, opened by three partial decryptions, exact");
}

int main()
{
    ckks();
    bfv();
    std::printf(failures ? "%d check(s) failed\n" : "all collective-refresh class-layer checks passed\n", failures);
    return failures ? 1 : 0;
}
