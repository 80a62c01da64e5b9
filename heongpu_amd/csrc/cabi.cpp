// cabi.cpp -- extern "C" entry points declared in include/hegpu.h.
#include "../../include/hegpu.h"
#include "../../include/hegpu_bench.h"
#include "context.hpp"
#include "encoding_transform.hpp"
#include "host_params.hpp"
#include "poly_eval.hpp"
#include "ops.hpp"
#include <cmath>
#include <complex>
#include <cstddef>
#include "tfhe.hpp"
#include <algorithm>
#include <cerrno>
#include <climits>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <cstring>
#include <functional>
#include <sys/random.h>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>

// The instrumented test build (tests/audit) compiles a fixed list of this directory's sources and must export every
// entry; it gets the host-only factorisation through this file instead of an object of its own.
#ifdef HEGPU_FP_AUDIT_HEADER
#include "encoding_transform.cpp"
#include "poly_eval.cpp"
#include "bootstrap_plan.cpp"
#endif

using namespace hegpu;

struct hegpu_context {
    Context c;
};

static thread_local std::string g_err;

static int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

// Every device entry point runs on the device its context was uploaded to, whatever the calling thread's current
// device is (one process driving several GPUs: one context per device, hegpu_context_upload_device); the thread's
// current device is restored on return.
struct DevGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess; // a failed switch is reported by the entry point (NEED_CTX / TFHE_NEED), never ignored:
                                 // the call would otherwise launch on the caller's device with another device's pointers
    explicit DevGuard(int dev)
    {
        if (dev < 0) return;
        if ((err = hipGetDevice(&prev)) != hipSuccess) return;
        if (prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DevGuard()
    {
        if (switched) (void) hipSetDevice(prev);
    }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};
static int hip_ret(hipError_t e, const char* where)
{
    if (e == hipSuccess) return 0;
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return (int) e;
}

template <typename F>
static int guarded(F&& f)
{
    try {
        return f();
    } catch (const std::invalid_argument& e) {
        return fail(HEGPU_E_INVALID, e.what());
    } catch (const std::logic_error& e) {
        return fail(HEGPU_E_LOGIC, e.what());
    } catch (const std::runtime_error& e) {
        return fail(HEGPU_E_RUNTIME, e.what());
    } catch (const std::bad_alloc&) {
        return fail(HEGPU_E_RUNTIME, "out of host memory");
    }
}

extern "C" {

const char* hegpu_last_error(void) { return g_err.c_str(); }
const char* hegpu_version(void) { return "hegpu-mi355x 0.1 (gfx950)"; }

// reference util.cu:11-56 coefficient_validator
static bool coefficient_validator(const int* q, int qn, const int* p, int pn)
{
    int total_p = 0;
    for (int i = 0; i < pn; i++) total_p += p[i];
    int idx = 0;
    for (int g = 0; g < qn / pn; g++) {
        int s = 0;
        for (int j = 0; j < pn; j++) s += q[idx++];
        if (s > total_p) return false;
    }
    int s = 0;
    for (int j = 0; j < qn % pn; j++) s += q[idx++];
    return s <= total_p;
}

static void check_degree(int n, int& n_power)
{
    if (n <= 0 || (n & (n - 1))) throw std::logic_error("Poly modulus degree have to be power of two");
    if (n > 65536 || n < 4096) throw std::logic_error("Poly modulus degree is not supported");
    n_power = 31 - __builtin_clz((unsigned) n);
}

// a modulus of at most 60 bits that admits a 2N-th root of unity
static void check_prime(uint64_t p, int n)
{
    if (p >> 61) throw std::logic_error("invalid modulus bit size");
    if ((p - 1) % (2 * (u64) n)) throw std::logic_error("no sufficient root unity");
}

// the total width of the chain against the security table (ckks/context.cu:94-119, secstdparams.h:25-79)
static void check_security(int n, int total_bits, int sec_level)
{
    if (sec_level == HEGPU_SEC_128 || sec_level == HEGPU_SEC_192 || sec_level == HEGPU_SEC_256) {
        if (host::max_logq((u64) n, sec_level) < total_bits)
            throw std::runtime_error("Parameters do not align with the security recommendations "
                                     "provided by the lattice-estimator");
    } else if (sec_level != HEGPU_SEC_NONE) {
        throw std::runtime_error("Invalid security level");
    }
}

static int finish_create(std::unique_ptr<hegpu_context> h, int scheme, int n_power, uint64_t plain_modulus, int q_count,
                         int p_count, hegpu_context** out)
{
    Context& c = h->c;
    c.scheme = scheme;
    c.n_power = n_power;
    c.Q_size = q_count;
    c.P_size = p_count;
    c.plain_modulus = plain_modulus;
    if (scheme == SCHEME_BFV && plain_modulus < 2) throw std::logic_error("plain modulus is not specified");
    c.build_host();
    c.seed_options_from_env(); // defaults only; hegpu_context_set_option is the interface
    *out = h.release();
    return 0;
}

int hegpu_context_create(int scheme, int n, const int* qb, int qn, const int* pb, int pn, uint64_t plain_modulus,
                         int sec_level, hegpu_context** out)
{
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("null output");
        if (scheme != SCHEME_BFV && scheme != SCHEME_CKKS) throw std::invalid_argument("unknown scheme");
        int n_power;
        check_degree(n, n_power);
        if (pn <= 0 || !pb) throw std::logic_error("log_P_bases_bit_sizes cannot be empty!");
        if (qn <= 0 || !qb) throw std::logic_error("log_Q_bases_bit_sizes cannot be empty!");
        if (!coefficient_validator(qb, qn, pb, pn)) throw std::logic_error("P should be bigger than Q pairs!");
        std::vector<int> bits(qb, qb + qn);
        bits.insert(bits.end(), pb, pb + pn);
        int total = 0;
        for (int b : bits) total += b;
        check_security(n, total, sec_level);
        std::unique_ptr<hegpu_context> h(new hegpu_context());
        h->c.primes = host::find_primes((u64) n, bits);
        return finish_create(std::move(h), scheme, n_power, plain_modulus, qn, pn, out);
    });
}

int hegpu_context_create_default(int scheme, int n, int p_count, uint64_t plain_modulus, int sec_level,
                                 hegpu_context** out)
{
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("null output");
        if (scheme != SCHEME_BFV && scheme != SCHEME_CKKS) throw std::invalid_argument("unknown scheme");
        int n_power;
        check_degree(n, n_power);
        if (p_count < 1) throw std::logic_error("P_modulus_size cannot be lower than 1!");
        if (sec_level != HEGPU_SEC_128 && sec_level != HEGPU_SEC_192 && sec_level != HEGPU_SEC_256)
            throw std::runtime_error("Invalid security level"); // bfv/context.cu:285-360: no default chain without a level
        std::vector<u64> chain = host::default_chain((u64) n, sec_level);
        if (chain.empty() || (int) chain.size() <= p_count) throw std::logic_error("no default chain");
        std::unique_ptr<hegpu_context> h(new hegpu_context());
        h->c.primes = chain;
        return finish_create(std::move(h), scheme, n_power, plain_modulus, (int) chain.size() - p_count, p_count, out);
    });
}

int hegpu_context_create_from_primes(int scheme, int n, const uint64_t* primes, int qn, int pn,
                                     uint64_t plain_modulus, hegpu_context** out)
{
    return guarded([&]() -> int {
        if (!out || !primes) throw std::invalid_argument("null argument");
        if (scheme != SCHEME_BFV && scheme != SCHEME_CKKS) throw std::invalid_argument("unknown scheme");
        int n_power;
        check_degree(n, n_power);
        if (pn <= 0 || qn <= 0) throw std::logic_error("log_P_bases_bit_sizes cannot be empty!");
        for (int i = 0; i < qn + pn; i++) check_prime(primes[i], n);
        std::unique_ptr<hegpu_context> h(new hegpu_context());
        h->c.primes.assign(primes, primes + qn + pn);
        return finish_create(std::move(h), scheme, n_power, plain_modulus, qn, pn, out);
    });
}

// set_coeff_modulus_values' own checks (bfv/context.cu:149-220, ckks/context.cu:149-220): every value admits a 2N-th
// root, the widths satisfy coefficient_validator, the total width respects the security table
int hegpu_validate_coeff_modulus_values(int n, const uint64_t* primes, int qn, int pn, int sec_level)
{
    return guarded([&]() -> int {
        if (!primes) throw std::invalid_argument("null argument");
        int n_power;
        check_degree(n, n_power);
        if (pn <= 0) throw std::logic_error("log_P_bases_bit_sizes cannot be empty!");
        if (qn <= 0) throw std::logic_error("log_Q_bases_bit_sizes cannot be empty!");
        std::vector<int> bits;
        int total = 0;
        for (int i = 0; i < qn + pn; i++) {
            if (primes[i] < 2) throw std::logic_error("invalid modulus bit size"); // (the constructor does not test this)
            check_prime(primes[i], n);
            bits.push_back(64 - __builtin_clzll(primes[i]));
            total += bits.back();
        }
        if (!coefficient_validator(bits.data(), qn, bits.data() + qn, pn))
            throw std::logic_error("Invalid parameters, P should be bigger than Q pairs!");
        check_security(n, total, sec_level);
        return 0;
    });
}

void hegpu_context_destroy(hegpu_context* ctx) { delete ctx; }

int hegpu_context_set_option(hegpu_context* ctx, const char* name, int value)
{
    if (!ctx || !name) return fail(HEGPU_E_INVALID, "null argument");
    switch (ctx->c.set_option(name, value)) {
        case 0: return 0;
        case 1: return fail(HEGPU_E_INVALID, std::string("unknown option: ") + name);
        case 2: return fail(HEGPU_E_INVALID, std::string("value out of range for option ") + name);
        default: return fail(HEGPU_E_LOGIC, std::string("option ") + name + " must be set before hegpu_context_upload");
    }
}

int hegpu_context_get_option(const hegpu_context* ctx, const char* name, int* value)
{
    if (!ctx || !name || !value) return fail(HEGPU_E_INVALID, "null argument");
    if (ctx->c.get_option(name, value)) return fail(HEGPU_E_INVALID, std::string("unknown option: ") + name);
    return 0;
}

// the number of HIP devices, at least one -- or the error every device entry point ends with on a box without one
static int need_device(int* cnt)
{
    if (hipGetDeviceCount(cnt) == hipSuccess && *cnt > 0) return 0;
    (void) hipGetLastError();
    return fail(HEGPU_E_NODEVICE, "no HIP device available: the HIP backend cannot run (no CPU fallback)");
}

int hegpu_context_upload(hegpu_context* ctx)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    int cnt = 0;
    if (int r = need_device(&cnt)) return r;
    return hip_ret(ctx->c.upload(), "context upload");
}

int hegpu_context_upload_device(hegpu_context* ctx, int device)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    int cnt = 0;
    if (int r = need_device(&cnt)) return r;
    if (device < 0 || device >= cnt) return fail(HEGPU_E_INVALID, "no such device");
    if (ctx->c.uploaded)
        return ctx->c.device == device ? 0 : fail(HEGPU_E_LOGIC, "the context is already uploaded to another device");
    DevGuard g(device);
    return hip_ret(ctx->c.upload(), "context upload");
}

int hegpu_context_device(const hegpu_context* ctx) { return (ctx && ctx->c.uploaded) ? ctx->c.device : -1; }

int hegpu_context_clone(const hegpu_context* src, hegpu_context** out)
{
    return guarded([&]() -> int {
        if (!src || !out) throw std::invalid_argument("null argument");
        std::unique_ptr<hegpu_context> h(new hegpu_context());
        // host state and options only: the clone owns its own device tables once uploaded
        static_cast<ContextHost&>(h->c) = src->c;
        *out = h.release();
        return 0;
    });
}

// Evaluation keys are the only data every GPU needs a copy of.  xGMI is point-to-point: on a fully
// connected node every destination has its own link to the source, so the replication is ONE hop -- a flat fan-out,
// every copy on its destination's stream, all links busy at once (272 MiB at ~50 GB/s per direction and link: ~5 ms).
// Where some destination is not directly reachable from the source (hipDeviceCanAccessPeer) the copies form a binomial
// tree (copy i -> i + 2^r in round r) cut into <= 32 MiB chunks, so that hop r + 1 of a chunk starts as soon as that
// chunk has arrived, not when the whole buffer has.  Peer access is enabled for every edge that is used; an edge
// without it is still copied (the runtime stages it through host memory) and reported (HEGPU_BCAST_STAGED).
static thread_local int g_bcast_path = 0;
int hegpu_last_broadcast_path(void) { return g_bcast_path; }

static const size_t kBcastChunk = (size_t) 32 << 20;

// 1: direct (same device, or peer access available and now enabled on `dst` for `src`), 0: not, <0: error in *e
static int peer_edge(int src, int dst, hipError_t* e)
{
    if (src == dst) return 1;
    int can = 0;
    if ((*e = hipDeviceCanAccessPeer(&can, dst, src)) != hipSuccess) return -1;
    if (!can) return 0;
    DevGuard g(dst);
    if (g.err != hipSuccess) {
        *e = g.err;
        return -1;
    }
    const hipError_t en = hipDeviceEnablePeerAccess(src, 0);
    if (en != hipSuccess && en != hipErrorPeerAccessAlreadyEnabled) {
        *e = en;
        return -1;
    }
    (void) hipGetLastError(); // "already enabled" is not an error to leave behind
    return 1;
}

int hegpu_broadcast_bytes(const int* devices, int n, void* const* bufs, size_t bytes, const hegpu_stream* streams,
                          int* path_out)
{
    g_bcast_path = 0;
    if (path_out) *path_out = 0;
    if (!devices || !bufs || n < 1) return fail(HEGPU_E_INVALID, "null argument");
    int cnt = 0;
    if (int r = need_device(&cnt)) return r;
    for (int i = 0; i < n; i++) {
        if (!bufs[i]) return fail(HEGPU_E_INVALID, "null buffer");
        if (devices[i] < 0 || devices[i] >= cnt) return fail(HEGPU_E_INVALID, "no such device");
    }
    if (n == 1 || bytes == 0) return 0;
    hipError_t e = hipSuccess;
    // ---- shape: flat when every destination is directly reachable from the source
    bool flat = true, same = true;
    for (int j = 1; j < n && flat; j++) {
        const int r = peer_edge(devices[0], devices[j], &e);
        if (r < 0) return hip_ret(e, "hegpu_broadcast: peer access");
        flat = r == 1;
    }
    for (int j = 1; j < n; j++) same = same && devices[j] == devices[0];
    std::vector<int> parent(n, 0);
    bool staged = false;
    if (!flat) {
        for (int span = 1; span < n; span <<= 1)
            for (int i = 0; i < span && i + span < n; i++) parent[i + span] = i;
        for (int j = 1; j < n; j++) {
            const int r = peer_edge(devices[parent[j]], devices[j], &e);
            if (r < 0) return hip_ret(e, "hegpu_broadcast: peer access");
            staged = staged || r == 0;
        }
    }
    // ---- copies: chunk c reaches node j on stream j, behind the event "chunk c complete at parent[j]"
    const size_t nchunks = (bytes + kBcastChunk - 1) / kBcastChunk;
    auto stream_of = [&](int i) { return streams ? (hipStream_t) streams[i] : (hipStream_t) nullptr; };
    std::vector<hipEvent_t> events;
    auto mark = [&](int i, hipEvent_t* ev) { // everything queued on stream i so far
        DevGuard g(devices[i]);
        if ((e = g.err) != hipSuccess) return;
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return;
        events.push_back(*ev);
        e = hipEventRecord(*ev, stream_of(i));
    };
    // arrived[j][c]; the source's one event covers all its chunks
    std::vector<std::vector<hipEvent_t>> arrived(n, std::vector<hipEvent_t>(nchunks, nullptr));
    hipEvent_t src_ready = nullptr;
    mark(0, &src_ready);
    for (size_t c = 0; c < nchunks; c++) arrived[0][c] = src_ready;
    // chunk-major order: a chunk walks down the tree before the next one is queued, so every stream sees its copies in
    // chunk order and a child never waits for more than the chunk it forwards
    for (size_t c = 0; c < nchunks && e == hipSuccess; c++) {
        const size_t off = c * kBcastChunk, len = std::min(kBcastChunk, bytes - off);
        for (int j = 1; j < n && e == hipSuccess; j++) { // parents precede children in index order
            const int pj = parent[j];
            DevGuard g(devices[j]);
            if ((e = g.err) != hipSuccess) break;
            if ((e = hipStreamWaitEvent(stream_of(j), arrived[pj][c], 0)) != hipSuccess) break;
            if ((e = hipMemcpyPeerAsync((char*) bufs[j] + off, devices[j], (const char*) bufs[pj] + off, devices[pj], len,
                                        stream_of(j))) != hipSuccess)
                break;
            bool has_child = false;
            for (int k = j + 1; k < n; k++) has_child = has_child || parent[k] == j;
            if (has_child) mark(j, &arrived[j][c]);
        }
    }
    for (hipEvent_t ev : events) (void) hipEventDestroy(ev); // released by the runtime once the recorded work has completed
    if (e != hipSuccess) return hip_ret(e, "hegpu_broadcast");
    int path = flat ? HEGPU_BCAST_FLAT : HEGPU_BCAST_TREE;
    if (staged) path |= HEGPU_BCAST_STAGED;
    if (same) path |= HEGPU_BCAST_SAME_DEVICE;
    g_bcast_path = path;
    if (path_out) *path_out = path;
    return 0;
}

int hegpu_broadcast_key(hegpu_context* const* ctxs, int n_ctx, uint64_t* const* keys, size_t elems,
                        const hegpu_stream* streams)
{
    g_bcast_path = 0;
    if (!ctxs || !keys || n_ctx < 1) return fail(HEGPU_E_INVALID, "null argument");
    std::vector<int> devs(n_ctx);
    std::vector<void*> bufs(n_ctx);
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i] || !keys[i]) return fail(HEGPU_E_INVALID, "null context or key pointer");
        if (!ctxs[i]->c.uploaded) return fail(HEGPU_E_LOGIC, "every context must be uploaded (hegpu_context_upload_device)");
        devs[i] = ctxs[i]->c.device;
        bufs[i] = keys[i];
    }
    return hegpu_broadcast_bytes(devs.data(), n_ctx, bufs.data(), elems * sizeof(u64), streams, nullptr);
}

long hegpu_context_int(const hegpu_context* ctx, const char* name)
{
    if (!ctx || !name) return -1;
    const Context& c = ctx->c;
    if (!strcmp(name, "n_power")) return c.n_power;
    if (!strcmp(name, "n")) return (long) c.n;
    if (!strcmp(name, "Q_size")) return c.Q_size;
    if (!strcmp(name, "P_size")) return c.P_size;
    if (!strcmp(name, "Q_prime_size")) return c.Qp_size;
    if (!strcmp(name, "bsk_modulus")) return c.bsk_size;
    if (!strcmp(name, "scheme")) return c.scheme;
    if (!strcmp(name, "max_logq_128")) return host::max_logq_128((int) c.n); // util/secstdparams.h
    if (!strcmp(name, "max_logq_192")) return host::max_logq(c.n, 192);
    if (!strcmp(name, "max_logq_256")) return host::max_logq(c.n, 256);
    return -1;
}

long hegpu_context_get(const hegpu_context* ctx, const char* name, uint64_t* out, long cap)
{
    if (!ctx || !name) return -1;
    auto it = ctx->c.host.find(name);
    if (it == ctx->c.host.end()) return -1;
    const long cnt = (long) it->second.size();
    if (!out) return cnt;
    if (cnt > cap) return -2;
    memcpy(out, it->second.data(), cnt * sizeof(uint64_t));
    return cnt;
}

const void* hegpu_context_device_ptr(const hegpu_context* ctx, const char* name)
{
    if (!ctx || !name) return nullptr;
    auto it = ctx->c.dev.find(name);
    return it == ctx->c.dev.end() ? nullptr : it->second;
}

int hegpu_steps_to_galois_elt(int steps, int coeff_count, int group_order)
{
    // no exception may cross the C boundary; Galois elements are odd and positive (0: step count out
    // of range, as the reference returns), so -1 is unambiguous
    int elt = -1;
    (void) guarded([&]() -> int {
        elt = host::steps_to_galois_elt(steps, coeff_count, group_order);
        return 0;
    });
    return elt;
}

// host only: the factors of the encoder's special FFT in diagonal form (encoding_transform.hpp)
static int log2_exact(int v)
{
    int p = 0;
    while ((1 << p) < v && p < 30) p++;
    return (v > 0 && (1 << p) == v) ? p : -1;
}

int hegpu_encoding_transform_shape(int coeff_count, int inverse, int pieces, int* strides, int* stages, int* n_diags)
{
    return guarded([&]() -> int {
        if (!strides || !stages || !n_diags) return fail(HEGPU_E_INVALID, "encoding_transform_shape: null argument");
        const int n_power = log2_exact(coeff_count);
        if (n_power < 0) return fail(HEGPU_E_INVALID, "encoding_transform_shape: the degree is a power of two");
        if (pieces < 1) return fail(HEGPU_E_INVALID, "encoding_transform_shape: the piece count lies in [2, 5]");
        for (int p = 0; p < pieces; p++) {
            const host::EncodingTransformPiece g = host::encoding_transform_piece(n_power, inverse != 0, pieces, p);
            strides[p] = g.stride;
            stages[p] = g.stages;
            n_diags[p] = (int) g.offsets.size();
        }
        return 0;
    });
}

int hegpu_encoding_transform_fill(int coeff_count, int inverse, int pieces, int piece, int n_diag, int* offsets,
                                  double* values)
{
    return guarded([&]() -> int {
        if (!offsets || !values) return fail(HEGPU_E_INVALID, "encoding_transform_fill: null argument");
        const int n_power = log2_exact(coeff_count);
        if (n_power < 0) return fail(HEGPU_E_INVALID, "encoding_transform_fill: the degree is a power of two");
        const host::EncodingTransformPiece g = host::encoding_transform_piece(n_power, inverse != 0, pieces, piece);
        if (n_diag != (int) g.offsets.size())
            return fail(HEGPU_E_INVALID, "encoding_transform_fill: n_diag is not what hegpu_encoding_transform_shape gives");
        const size_t n = (size_t) coeff_count >> 1;
        for (size_t d = 0; d < g.offsets.size(); d++) {
            offsets[d] = g.offsets[d];
            for (size_t t = 0; t < n; t++) {
                values[2 * (d * n + t)] = g.diags[d][t].real();
                values[2 * (d * n + t) + 1] = g.diags[d][t].imag();
            }
        }
        return 0;
    });
}

int hegpu_giant_step_chain(const int* giant_shifts, int n2, int slots, int* parent, int* link_shifts)
{
    return guarded([&]() -> int {
        host::giant_step_chain(giant_shifts, n2, slots, parent, link_shifts);
        return 0;
    });
}

// host only: the step plans (poly_eval.hpp) and the refresh plans (bootstrap_plan.hpp).  The three step-plan families
// share one size and one fill: `make` is the family's planner over the caller's arguments, `who` the name in the messages.
using MakePlan = std::function<std::vector<host::PolyStep>()>;
static int plan_size(const MakePlan& make, const char* who, int* n_steps)
{
    return guarded([&]() -> int {
        if (!n_steps) return fail(HEGPU_E_INVALID, std::string(who) + "_size: null argument");
        *n_steps = (int) make().size();
        return 0;
    });
}

static int plan_fill(const MakePlan& make, const char* who, hegpu_poly_step* steps, int n_steps)
{
    return guarded([&]() -> int {
        if (!steps) return fail(HEGPU_E_INVALID, std::string(who) + "_fill: null argument");
        const std::vector<host::PolyStep> plan = make();
        if (n_steps != (int) plan.size())
            return fail(HEGPU_E_INVALID, std::string(who) + "_fill: n_steps is not what hegpu_" + who + "_size gives");
        std::copy(plan.begin(), plan.end(), steps);
        return 0;
    });
}

static std::vector<uint64_t> primes_of(const uint64_t* primes, int n_primes, const char* who)
{
    if (!primes || n_primes < 1) throw std::invalid_argument(std::string(who) + ": null argument");
    return std::vector<uint64_t>(primes, primes + n_primes);
}

static std::vector<host::PolyStep> poly_plan_of(int basis, const double* coeffs, int n_coeffs, int max_deg, int lead, int level,
                                                double scale, double target_scale, const uint64_t* primes, int n_primes)
{
    if (!coeffs || !primes) throw std::invalid_argument("poly_eval_plan: null argument");
    if (n_coeffs < 1 || n_primes < 1) throw std::invalid_argument("poly_eval_plan: the degree is at least 2");
    std::vector<std::complex<double>> c((size_t) n_coeffs);
    for (int i = 0; i < n_coeffs; i++) c[(size_t) i] = std::complex<double>(coeffs[2 * i], coeffs[2 * i + 1]);
    return host::poly_eval_plan(basis, c, max_deg, lead != 0, level, scale, target_scale,
                                std::vector<uint64_t>(primes, primes + n_primes));
}

int hegpu_poly_eval_plan_size(int basis, const double* coeffs, int n_coeffs, int max_deg, int lead, int level, double scale,
                              double target_scale, const uint64_t* primes, int n_primes, int* n_steps)
{
    return plan_size([&] { return poly_plan_of(basis, coeffs, n_coeffs, max_deg, lead, level, scale, target_scale, primes, n_primes); },
                     "poly_eval_plan", n_steps);
}

int hegpu_poly_eval_plan_fill(int basis, const double* coeffs, int n_coeffs, int max_deg, int lead, int level, double scale,
                              double target_scale, const uint64_t* primes, int n_primes, hegpu_poly_step* steps, int n_steps)
{
    return plan_fill([&] { return poly_plan_of(basis, coeffs, n_coeffs, max_deg, lead, level, scale, target_scale, primes, n_primes); },
                     "poly_eval_plan", steps, n_steps);
}

int hegpu_eval_mod_plan_size(int K, int degree, int double_angle, int level, double scale, double target_scale,
                             const uint64_t* primes, int n_primes, int* n_steps)
{
    return plan_size([&] { return host::eval_mod_plan(K, degree, double_angle, level, scale, target_scale,
                                                      primes_of(primes, n_primes, "eval_mod_plan")); },
                     "eval_mod_plan", n_steps);
}

int hegpu_eval_mod_plan_fill(int K, int degree, int double_angle, int level, double scale, double target_scale,
                             const uint64_t* primes, int n_primes, hegpu_poly_step* steps, int n_steps)
{
    return plan_fill([&] { return host::eval_mod_plan(K, degree, double_angle, level, scale, target_scale,
                                                      primes_of(primes, n_primes, "eval_mod_plan")); },
                     "eval_mod_plan", steps, n_steps);
}

int hegpu_eval_trig_plan_size(int K, int degree, int double_angle, double phase, double amplitude, double offset, int level,
                              double scale, double target_scale, const uint64_t* primes, int n_primes, int* n_steps)
{
    return plan_size([&] { return host::eval_trig_plan(K, degree, double_angle, phase, amplitude, offset, level, scale, target_scale,
                                                       primes_of(primes, n_primes, "eval_trig_plan")); },
                     "eval_trig_plan", n_steps);
}

int hegpu_eval_trig_plan_fill(int K, int degree, int double_angle, double phase, double amplitude, double offset, int level,
                              double scale, double target_scale, const uint64_t* primes, int n_primes,
                              hegpu_poly_step* steps, int n_steps)
{
    return plan_fill([&] { return host::eval_trig_plan(K, degree, double_angle, phase, amplitude, offset, level, scale, target_scale,
                                                       primes_of(primes, n_primes, "eval_trig_plan")); },
                     "eval_trig_plan", steps, n_steps);
}

int hegpu_bootstrap_plan_fill(const hegpu_bootstrap_config* config, const uint64_t* primes, int n_primes, hegpu_bootstrap_plan* plan)
{
    return guarded([&]() -> int {
        if (!config || !primes || !plan || n_primes < 1) return fail(HEGPU_E_INVALID, "bootstrap_plan_fill: null argument");
        *plan = host::bootstrap_plan(*config, std::vector<uint64_t>(primes, primes + n_primes));
        return 0;
    });
}

int hegpu_slim_bootstrap_plan_fill(const hegpu_slim_bootstrap_config* config, const uint64_t* primes, int n_primes,
                                   hegpu_slim_bootstrap_plan* plan)
{
    return guarded([&]() -> int {
        if (!config || !primes || !plan || n_primes < 1) return fail(HEGPU_E_INVALID, "slim_bootstrap_plan_fill: null argument");
        *plan = host::slim_bootstrap_plan(*config, std::vector<uint64_t>(primes, primes + n_primes));
        return 0;
    });
}

#define NEED_CTX(ctx)                                                                      \
    if (!(ctx)) return fail(HEGPU_E_INVALID, "null context");                              \
    if (!(ctx)->c.uploaded) {                                                              \
        int r__ = hegpu_context_upload(ctx);                                               \
        if (r__) return r__;                                                               \
    }                                                                                      \
    DevGuard dev_guard__((ctx)->c.device);                                                 \
    if (dev_guard__.err != hipSuccess) return hip_ret(dev_guard__.err, "switching to the context's device")

static const Mod* mods_of(const Context& c, int table_set)
{
    return table_set == HEGPU_TABLES_Q_BSK ? c.plan_merge.mods : c.plan_qp.mods;
}

int hegpu_ntt(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int inverse, int batch,
              int mod_count, int mod_offset, const int* mod_order, const int* poly_order, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (table_set == HEGPU_TABLES_Q_BSK && c.scheme != SCHEME_BFV)
        return fail(HEGPU_E_INVALID, "q|Bsk tables exist only in a BFV context");
    if (table_set < 0 || table_set > HEGPU_TABLES_PLAIN || (table_set == HEGPU_TABLES_PLAIN && !c.plan_plain.count))
        return fail(HEGPU_E_INVALID, "no such table set in this context");
    NttArgs a = c.ntt_args(table_set);
    const int avail = a.mod_count;
    if (mod_count <= 0 || mod_offset < 0 || (!mod_order && mod_offset + mod_count > avail))
        return fail(HEGPU_E_INVALID, "modulus range outside the table set");
    a.in = (const u64*) in;
    a.out = (u64*) out;
    a.mod_count = mod_count;
    a.mod_offset = mod_offset;
    a.mod_order = mod_order;
    a.poly_order = poly_order;
    return hip_ret(ntt_launch(a, batch, inverse != 0, (hipStream_t) stream), "hegpu_ntt");
}

// the six gpuntt:: names (include/hegpu.h)
int hegpu_GPU_NTT(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int mod_offset, int batch,
                  int mod_count, hegpu_stream stream)
{
    return hegpu_ntt(ctx, table_set, in, out, 0, batch, mod_count, mod_offset, nullptr, nullptr, stream);
}
int hegpu_GPU_NTT_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int mod_offset, int batch, int mod_count,
                          hegpu_stream stream)
{
    return hegpu_ntt(ctx, table_set, inout, inout, 0, batch, mod_count, mod_offset, nullptr, nullptr, stream);
}
int hegpu_GPU_INTT(hegpu_context* ctx, int table_set, const uint64_t* in, uint64_t* out, int mod_offset, int batch,
                   int mod_count, hegpu_stream stream)
{
    return hegpu_ntt(ctx, table_set, in, out, 1, batch, mod_count, mod_offset, nullptr, nullptr, stream);
}
int hegpu_GPU_INTT_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int mod_offset, int batch,
                           int mod_count, hegpu_stream stream)
{
    return hegpu_ntt(ctx, table_set, inout, inout, 1, batch, mod_count, mod_offset, nullptr, nullptr, stream);
}
int hegpu_GPU_NTT_Modulus_Ordered_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int inverse,
                                          int mod_offset, int batch, int mod_count, const int* order,
                                          hegpu_stream stream)
{
    if (!order) return fail(HEGPU_E_INVALID, "modulus order table is required");
    return hegpu_ntt(ctx, table_set, inout, inout, inverse, batch, mod_count, mod_offset, order, nullptr, stream);
}
int hegpu_GPU_NTT_Poly_Ordered_Inplace(hegpu_context* ctx, int table_set, uint64_t* inout, int inverse, int mod_offset,
                                       int batch, int mod_count, const int* order, hegpu_stream stream)
{
    if (!order) return fail(HEGPU_E_INVALID, "polynomial order table is required");
    return hegpu_ntt(ctx, table_set, inout, inout, inverse, batch, mod_count, mod_offset, nullptr, order, stream);
}

int hegpu_addition(hegpu_context* ctx, const uint64_t* in1, const uint64_t* in2, uint64_t* out, int limbs,
                   int parts, int batch, int op, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (limbs <= 0 || limbs > c.Qp_size || op < 0 || op > 2) return fail(HEGPU_E_INVALID, "bad limbs/op");
    return hip_ret(rns_addition((const u64*) in1, (const u64*) in2, (u64*) out, c.plan_qp.mods, c.n_power, limbs,
                                parts, batch, op, (hipStream_t) stream),
                   "hegpu_addition");
}

int hegpu_cross_multiplication(hegpu_context* ctx, int table_set, const uint64_t* in1, uint64_t s1,
                               const uint64_t* in2, uint64_t s2, uint64_t* out, uint64_t so, int decomp_size,
                               int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    const Mod* m = mods_of(c, table_set);
    if (!m) return fail(HEGPU_E_INVALID, "table set not available");
    return hip_ret(rns_cross_multiplication((const u64*) in1, s1, (const u64*) in2, s2, (u64*) out, so, m, c.n_power,
                                            decomp_size, batch, (hipStream_t) stream),
                   "hegpu_cross_multiplication");
}

int hegpu_cipher_broadcast(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                           uint64_t out_stride, int digits, int nmods, int split, int level, int batch,
                           hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    return hip_ret(rns_decompose((const u64*) in, in_stride, (u64*) out, out_stride, c.plan_qp.mods, c.n_power,
                                 digits, nmods, split, level, batch, (hipStream_t) stream),
                   "hegpu_cipher_broadcast");
}

int hegpu_keyswitch_multiply_accumulate(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride,
                                        const uint64_t* key, uint64_t* out, uint64_t out_stride, int digits,
                                        int nmods, int key_limbs, int split, int level, int batch,
                                        hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    return hip_ret(rns_keyswitch_mac((const u64*) in, in_stride, (const u64*) key, (u64*) out, out_stride,
                                     c.plan_qp.mods, c.n_power, digits, nmods, key_limbs, split, level, batch,
                                     (hipStream_t) stream),
                   "hegpu_keyswitch_multiply_accumulate");
}

int hegpu_base_conversion_DtoQtilde(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                                    uint64_t out_stride, int depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (c.P_size < 2) return fail(HEGPU_E_LOGIC, "method II tables exist only when P_size > 1");
    if (depth < 0 || depth >= (int) c.m2_levels.size()) return fail(HEGPU_E_INVALID, "invalid depth");
    const Context::M2Level& L = c.m2_levels[depth];
    return hip_ret(rns_base_conversion_DtoQtilde((const u64*) in, in_stride, (u64*) out, out_stride, c.plan_qp.mods,
                                                 c.tab.m2_matrix_mg + L.off_matrix, c.tab.m2_Mi_inv + L.off_mi,
                                                 c.tab.m2_negprod_mg + L.off_prod, c.tab.m2_I_j + L.off_digits,
                                                 c.tab.m2_I_location + L.off_digits, c.n_power, L.d, L.rc,
                                                 c.Q_size - depth, depth, c.m2_width, batch, (hipStream_t) stream),
                   "hegpu_base_conversion_DtoQtilde");
}

int hegpu_divide_round_lastq(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                             uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int switchkey, int batch,
                             hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (c.P_size != 1) return fail(HEGPU_E_LOGIC, "divide_round_lastq needs a single special prime (method I)");
    return hip_ret(rns_divide_round_lastq((const u64*) in, in_stride, (const u64*) ct, ct_stride, (u64*) out,
                                          out_stride, c.moddown(0), switchkey, batch, (hipStream_t) stream),
                   "hegpu_divide_round_lastq");
}

int hegpu_divide_round_lastq_permute(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride,
                                     const uint64_t* in2, uint64_t in2_stride, uint64_t* out,
                                     uint64_t out_stride, int galois_elt, int depth, int batch,
                                     hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (c.scheme == SCHEME_BFV && depth != 0) return fail(HEGPU_E_INVALID, "BFV ciphertexts have no depth");
    return hip_ret(rns_moddown_permute((const u64*) in, in_stride, (const u64*) in2, in2_stride, (u64*) out,
                                       out_stride, c.moddown(depth), galois_elt, batch, (hipStream_t) stream),
                   "hegpu_divide_round_lastq_permute");
}

// ------------------------------------------------------------------ the argument rules the entry points share
// Every check_* below returns 0 (go on), the code of a refusal whose message fail() has stored, or EMPTY_BATCH: the call
// is a no-op and the entry returns 0 at once.  An entry uses them as `if (int r = check_x(...)) return leave(r);`, or
// `return r;` where the check has no empty-batch exit.  EMPTY_BATCH is negative: no HEGPU_E_* code and no hipError_t is.
static const int EMPTY_BATCH = -1;
static int leave(int r) { return r == EMPTY_BATCH ? 0 : r; }
static int require(bool ok, const std::string& msg) { return ok ? 0 : fail(HEGPU_E_INVALID, msg); }
static int check_scheme(const Context& c, int want) { return require(c.scheme == want, "context scheme mismatch"); }
static int check_batch(int batch) // its sign, and the empty batch: the entry returns leave(r)
{
    if (batch < 0) return fail(HEGPU_E_INVALID, "batch must not be negative");
    return batch == 0 ? EMPTY_BATCH : 0;
}
static int check_grid(int batch, int k, const char* who) // a grid dimension holds 65535 blocks, the entry launches k per item
{
    if (k * (long) batch <= 65535) return 0;
    return fail(HEGPU_E_INVALID, std::string(who) + ": at most " + std::to_string(65535 / k) + " items per call");
}
static int check_items(int batch, int k, const char* who) // the entries for which an empty batch is a refusal
{
    if (batch < 1) return fail(HEGPU_E_INVALID, std::string(who) + ": batch must be at least 1");
    return check_grid(batch, k, who);
}
static int check_depth(const Context& c, int depth) { return require(depth >= 0 && depth < c.Q_size, "invalid depth"); }
static int check_workspace(const void* ws, size_t have, size_t need) { return require(ws && have >= need, "workspace too small"); }
// The entries a caller's capture must not record.  One that draws randomness advances its generator's counter on the host:
// captured once and replayed, it would hand every replay the same (seed, counter) -- the same a, noise and u.  One that
// synchronises invalidates the capture.  Asked first: before anything is queued and before the counter moves.
static const char* const DRAWS = "draws randomness, and every replay would draw the same";
static const char* const SYNCS = "synchronises, which a capture does not allow";
static int check_not_capturing(hegpu_stream stream, const char* who, const char* why)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing((hipStream_t) stream, &status);
    if (e != hipSuccess) return hip_ret(e, who);
    if (status == hipStreamCaptureStatusNone) return 0;
    return fail(HEGPU_E_LOGIC, std::string(who) + ": the stream is being captured and this entry " + why +
                                   "; call it outside the capture");
}
// words of a ciphertext of `parts` polynomials at `limbs` limbs
static uint64_t ct_words(const Context& c, int limbs, int parts = 2) { return (uint64_t) parts * limbs * c.n; }
static uint64_t level_words(const Context& c, int depth) { return ct_words(c, c.Q_size - depth); } // two parts at `depth`
static bool galois_elt_ok(const Context& c, int e) { return e > 0 && (e & 1) && e < 2 * (int) c.n; }
// a list of rotations: element 0 is the identity and needs no key
static int check_galois_list(const Context& c, const uint64_t* const* keys, const int* elts, int count, const char* who)
{
    for (int i = 0; i < count; i++) {
        if (elts[i] == 0) continue;
        if (!galois_elt_ok(c, elts[i]))
            return fail(HEGPU_E_INVALID, std::string(who) + ": Galois elements are odd and below 2N");
        if (!keys[i]) return fail(HEGPU_E_INVALID, std::string(who) + ": Galois key not present!");
    }
    return 0;
}
// the baby-step / giant-step shape: 16 products per 128-bit sum, 256 indices by value
static bool bsgs_shape_ok(int n1, int n2) { return n1 >= 1 && n1 <= 16 && n2 >= 1 && n2 <= 16; }
// the parent table of chained giant steps (null, or all -1: the direct mode); after check_galois_list of the giant steps
static int check_giant_chain(const int* parent, int n2, const uint64_t* const* keys, const int* elts, const char* who)
{
    const char* why = ops_giant_chain_check(parent, n2, (const u64* const*) keys, elts);
    return why ? fail(HEGPU_E_INVALID, std::string(who) + ": " + why) : 0;
}
static int check_diag_index(const int* index, int n1, int n2, int n_diag, const char* who) // [n2][n1]: a packed diagonal or -1
{
    for (int k = 0; k < n1 * n2; k++)
        if (index[k] < -1 || index[k] >= n_diag)
            return fail(HEGPU_E_INVALID, std::string(who) + ": index outside [-1, n_diag)");
    return 0;
}
static int check_leaf_weights(const host::PolyStep* p, int n_steps, const char* who) // the constant term included
{
    for (int k = 0; k < n_steps; k++) {
        if (p[k].kind != host::POLY_STEP_LEAF) continue;
        for (int i = 0; i <= p[k].n_terms; i++) {
            const double* w = i < p[k].n_terms ? p[k].w[i] : p[k].w0;
            if (!std::isfinite(w[0]) || !std::isfinite(w[1]))
                return fail(HEGPU_E_INVALID, std::string(who) + ": a weight is not a finite number");
        }
    }
    return 0;
}
// a constant the kernels round to an integer: a number, and inside the range of a float
static bool constant_in_range(double v) { return v == v && v < 3.4e38 && v > -3.4e38; }
static int check_shape(const Context& c, int limbs, int parts) // a ciphertext on the Q chain
{
    return require(limbs > 0 && limbs <= c.Q_size && parts >= 2 && parts <= 3, "bad ciphertext shape");
}
// the leveled seam entries: a CKKS context, at least min_limbs limbs left at `depth`, then the batch
static int check_seam_ckks(const Context& c, int depth, int batch, int min_limbs)
{
    if (c.scheme != SCHEME_CKKS) return fail(HEGPU_E_INVALID, "CKKS context required");
    if (depth < 0 || c.Q_size - depth < min_limbs) return fail(HEGPU_E_INVALID, "invalid depth");
    return check_batch(batch);
}

int hegpu_divide_round_lastq_leveled_stage_one(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                                               uint64_t out_stride, int rescale, int depth, int batch,
                                               hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_seam_ckks(ctx->c, depth, batch, rescale ? 2 : 1)) return leave(r);
    if (!rescale && ctx->c.P_size != 1) return fail(HEGPU_E_LOGIC, "the leveled stages serve a single special prime (method I)");
    return hip_ret(rns_moddown_stage_one((const u64*) in, in_stride, (u64*) out, out_stride, ctx->c.moddown(depth, rescale != 0),
                                         batch, (hipStream_t) stream),
                   "hegpu_divide_round_lastq_leveled_stage_one");
}

int hegpu_divide_round_lastq_leveled_stage_two(hegpu_context* ctx, const uint64_t* in_last, uint64_t last_stride,
                                               const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                                               uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int switchkey,
                                               int depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_seam_ckks(ctx->c, depth, batch, 1)) return leave(r);
    if (ctx->c.P_size != 1) return fail(HEGPU_E_LOGIC, "the leveled stages serve a single special prime (method I)");
    if (!ct) return fail(HEGPU_E_INVALID, "ct must not be NULL");
    return hip_ret(rns_moddown_stage_two((const u64*) in_last, last_stride, (const u64*) in, in_stride, (const u64*) ct,
                                         ct_stride, (u64*) out, out_stride, ctx->c.moddown(depth), switchkey ? 2 : 1, batch,
                                         (hipStream_t) stream),
                   "hegpu_divide_round_lastq_leveled_stage_two");
}

int hegpu_move_cipher_leveled(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out,
                              uint64_t out_stride, int depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_seam_ckks(ctx->c, depth, batch, 2)) return leave(r);
    const int l = ctx->c.Q_size - depth;
    return hip_ret(rns_copy_limbs((const u64*) in, ct_words(ctx->c, l, 1), in_stride, (u64*) out, ct_words(ctx->c, l, 1),
                                  out_stride, ctx->c.n_power, l - 1, 2, batch, (hipStream_t) stream),
                   "hegpu_move_cipher_leveled");
}

int hegpu_divide_round_lastq_rescale(hegpu_context* ctx, const uint64_t* in_last, uint64_t last_stride,
                                     const uint64_t* in, uint64_t in_stride, uint64_t* out, uint64_t out_stride,
                                     int depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_seam_ckks(ctx->c, depth, batch, 2)) return leave(r);
    return hip_ret(rns_moddown_stage_two((const u64*) in_last, last_stride, (const u64*) in, in_stride, nullptr, 0,
                                         (u64*) out, out_stride, ctx->c.moddown(depth, true), 0, batch, (hipStream_t) stream),
                   "hegpu_divide_round_lastq_rescale");
}

int hegpu_divide_round_lastq_extended(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, const uint64_t* ct,
                                      uint64_t ct_stride, uint64_t* out, uint64_t out_stride, int mode, int depth,
                                      int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (mode < 0 || mode > 2) return fail(HEGPU_E_INVALID, "mode must be 0, 1 or 2");
    if (c.scheme == SCHEME_BFV && depth != 0) return fail(HEGPU_E_INVALID, "BFV ciphertexts have no depth");
    if (int r = check_depth(c, depth)) return r;
    if (mode && !ct) return fail(HEGPU_E_INVALID, "ct must not be NULL");
    if (int r = check_batch(batch)) return leave(r);
    return hip_ret(rns_moddown_extended((const u64*) in, in_stride, (const u64*) ct, ct_stride, (u64*) out, out_stride,
                                        c.moddown(depth), mode, batch, (hipStream_t) stream),
                   "hegpu_divide_round_lastq_extended");
}

int hegpu_fast_convertion(hegpu_context* ctx, const uint64_t* in1, uint64_t s1, const uint64_t* in2, uint64_t s2,
                          uint64_t* out, uint64_t so, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (c.scheme != SCHEME_BFV) return fail(HEGPU_E_INVALID, "BFV context required");
    return hip_ret(rns_fast_convertion((const u64*) in1, s1, (const u64*) in2, s2, (u64*) out, so, c.behz,
                                       c.n_power, batch, (hipStream_t) stream),
                   "hegpu_fast_convertion");
}

int hegpu_fast_floor(hegpu_context* ctx, const uint64_t* in, uint64_t si, uint64_t* out, uint64_t so, int batch,
                     hegpu_stream stream)
{
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    if (c.scheme != SCHEME_BFV) return fail(HEGPU_E_INVALID, "BFV context required");
    return hip_ret(rns_fast_floor((const u64*) in, si, (u64*) out, so, c.behz, c.n_power, batch,
                                  (hipStream_t) stream),
                   "hegpu_fast_floor");
}

// include/hegpu.h and ops.hpp number the workspace rows separately
#define SAME_OP(name) static_assert((int) HEGPU_OP_##name == (int) OP_##name, "HEGPU_OP_" #name " != OP_" #name)
SAME_OP(CKKS_RELIN); SAME_OP(CKKS_RESCALE); SAME_OP(CKKS_GALOIS); SAME_OP(BFV_MULTIPLY); SAME_OP(BFV_RELIN);
SAME_OP(BFV_GALOIS); SAME_OP(KEYGEN_SECRET); SAME_OP(KEYGEN_PUBLIC); SAME_OP(KEYGEN_SWITCH); SAME_OP(CKKS_ENCRYPT);
SAME_OP(BFV_ENCRYPT); SAME_OP(BFV_DECRYPT); SAME_OP(BFV_DECODE); SAME_OP(CKKS_ENCODE); SAME_OP(CKKS_DECODE);
SAME_OP(BFV_MULTIPLY_PLAIN); SAME_OP(CKKS_ROTATE_HOISTED); SAME_OP(MPC_KEY_SHARE); SAME_OP(MPC_BFV_DECRYPT_MERGE);
SAME_OP(MPC_REFRESH_SHARE); SAME_OP(MPC_REFRESH_MERGE); SAME_OP(CKKS_LOGIC_GATE); SAME_OP(BFV_LOGIC_GATE); SAME_OP(CKKS_MOD_RAISE);
SAME_OP(CKKS_BOOTSTRAP);
#undef SAME_OP

size_t hegpu_workspace_bytes(const hegpu_context* ctx, int op, int depth, int batch)
{
    if (!ctx || batch <= 0) return 0;
    return ops_workspace_elems(ctx->c, op, depth, batch) * sizeof(u64);
}

// the operators: scheme, batch (an empty batch is a no-op), depth, and the workspace row `op` (0: the entry has none, or
// sizes its workspace itself)
static int check_op(const hegpu_context* ctx, int want_scheme, int op, int depth, int batch, const void* ws, size_t ws_bytes)
{
    if (int r = check_scheme(ctx->c, want_scheme)) return r;
    if (int r = check_batch(batch)) return r;
    if (int r = check_depth(ctx->c, depth)) return r;
    return op ? check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, op, depth, batch)) : 0;
}

int hegpu_ckks_multiply(hegpu_context* ctx, const uint64_t* ct1, uint64_t s1, const uint64_t* ct2, uint64_t s2,
                        uint64_t* out, uint64_t so, int depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_depth(ctx->c, depth)) return r;
    return hip_ret(op_ckks_multiply(ctx->c, (const u64*) ct1, s1, (const u64*) ct2, s2, (u64*) out, so, depth, batch,
                                    (hipStream_t) stream),
                   "hegpu_ckks_multiply");
}

int hegpu_ckks_relinearize_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t cs, const uint64_t* key, int depth,
                                   int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, OP_CKKS_RELIN, depth, batch, ws, ws_bytes)) return leave(r);
    return hip_ret(op_ckks_relinearize(ctx->c, (u64*) ct, cs, (const u64*) key, depth, batch, (u64*) ws,
                                       (hipStream_t) stream),
                   "hegpu_ckks_relinearize_inplace");
}

int hegpu_probe_ckks_relinearize(hegpu_context* ctx, uint64_t* ct, uint64_t cs, const uint64_t* key, int depth,
                                 int batch, void* ws, size_t ws_bytes, unsigned phases, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, OP_CKKS_RELIN, depth, batch, ws, ws_bytes)) return leave(r);
    if (ctx->c.P_size != 1) return fail(HEGPU_E_LOGIC, "the phase probe covers key-switching method I");
    return hip_ret(op_ckks_relinearize(ctx->c, (u64*) ct, cs, (const u64*) key, depth, batch, (u64*) ws,
                                       (hipStream_t) stream, phases),
                   "hegpu_probe_ckks_relinearize");
}

void hegpu_probe_ks_launch_forms(uint64_t counts[3])
{
    unsigned long long c[3];
    ks_row_mac_launch_counts(c);
    for (int i = 0; i < 3; i++) counts[i] = c[i];
}

int hegpu_ckks_rescale_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t cs, int depth, int batch, void* ws,
                               size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, OP_CKKS_RESCALE, depth, batch, ws, ws_bytes)) return leave(r);
    if (depth >= ctx->c.Q_size - 1) return fail(HEGPU_E_LOGIC, "no modulus left to rescale by");
    return hip_ret(op_ckks_rescale(ctx->c, (u64*) ct, cs, depth, batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_ckks_rescale_inplace");
}

// The rotations read the input ciphertext while their epilogue already writes (scatters) results: no item of the result
// batch may share a word with an item of the input batch.  Items: [p + i * stride, + item) for i < batch, so layouts in
// which the two batches interleave without touching (ct and out alternating in one buffer, stride 2 * words) are fine.
// Equal strides: item i of a and item j of b overlap iff -b_item < (b - a) + (j - i) * stride < a_item -- one test per
// difference j - i.  Unequal strides: pairwise up to 1024 items, beyond that the whole spans (conservative).
static bool spans_overlap(const uint64_t* a, uint64_t a_stride, uint64_t a_item, const uint64_t* b, uint64_t b_stride,
                          uint64_t b_item, int batch)
{
    if (batch <= 0) return false;
    const __int128 W = sizeof(uint64_t);
    const __int128 a0 = (__int128) (uintptr_t) a, b0 = (__int128) (uintptr_t) b;
    const __int128 ai = (__int128) a_item * W, bi = (__int128) b_item * W;
    auto hit = [&](__int128 pa, __int128 pb) { return pa < pb + bi && pb < pa + ai; };
    if (batch == 1) return hit(a0, b0);
    {   // the whole spans first: disjoint buffers (the common case) need no per-item test
        const __int128 a1 = a0 + ((__int128) (batch - 1) * a_stride + a_item) * W;
        const __int128 b1 = b0 + ((__int128) (batch - 1) * b_stride + b_item) * W;
        if (!(a0 < b1 && b0 < a1)) return false;
    }
    if (a_stride == b_stride) {
        const __int128 st = (__int128) a_stride * W;
        for (long k = -(long) (batch - 1); k <= (long) (batch - 1); k++)
            if (hit(a0, b0 + k * st)) return true;
        return false;
    }
    if (batch <= 1024) {
        for (int i = 0; i < batch; i++)
            for (int j = 0; j < batch; j++)
                if (hit(a0 + (__int128) i * a_stride * W, b0 + (__int128) j * b_stride * W)) return true;
        return false;
    }
    return true; // beyond 1024 items with unequal strides: intersecting spans count as overlap (conservative)
}

// one batch of equally sized items: item i is [p + i * stride, + item)
struct Span {
    const uint64_t* p;
    uint64_t stride, item;
};

// `out` shares a word with one of `ins`
static bool overlaps_any(const Span& out, std::initializer_list<Span> ins, int batch)
{
    for (const Span& in : ins)
        if (spans_overlap(in.p, in.stride, in.item, out.p, out.stride, out.item, batch)) return true;
    return false;
}

int hegpu_ckks_apply_galois(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                            const uint64_t* key, int galois_elt, int depth, int batch, void* ws, size_t ws_bytes,
                            hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, OP_CKKS_GALOIS, depth, batch, ws, ws_bytes)) return leave(r);
    const uint64_t words = level_words(ctx->c, depth);
    if (spans_overlap(ct, cs, words, out, so, words, batch))
        return fail(HEGPU_E_INVALID, "apply_galois: out must not alias ct (the result buffer must not contain the input)");
    if (!galois_elt_ok(ctx->c, galois_elt))
        return fail(HEGPU_E_INVALID, "apply_galois: Galois elements are odd and below 2N");
    return hip_ret(op_ckks_apply_galois(ctx->c, (const u64*) ct, cs, (u64*) out, so, (const u64*) key, galois_elt, depth,
                                        batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_ckks_apply_galois");
}

// ---- the modulus raise.  Everything is checked on the host tables, before the context is uploaded: a refusal needs no device.
int hegpu_mod_raise(hegpu_context* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out, uint64_t out_stride,
                    int limbs, int parts, int batch, hegpu_stream stream)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    if (!in || !out) return fail(HEGPU_E_INVALID, "mod_raise: null argument");
    if (batch < 1 || batch > 65535) return fail(HEGPU_E_INVALID, "mod_raise: 1 to 65535 items per call");
    if (parts < 1 || parts > 3) return fail(HEGPU_E_INVALID, "mod_raise: parts is 1, 2 or 3");
    if (limbs < 1 || limbs > ctx->c.Q_size) return fail(HEGPU_E_INVALID, "mod_raise: 1 <= limbs <= Q");
    if (spans_overlap(in, in_stride, ct_words(ctx->c, 1, parts), out, out_stride, ct_words(ctx->c, limbs, parts), batch))
        return fail(HEGPU_E_INVALID, "mod_raise: out must not overlap in");
    NEED_CTX(ctx);
    const Context& c = ctx->c;
    return hip_ret(rns_mod_raise((const u64*) in, in_stride, (u64*) out, out_stride, c.plan_qp.mods, c.n_power, limbs, parts,
                                 batch, (hipStream_t) stream),
                   "hegpu_mod_raise");
}

int hegpu_ckks_mod_raise(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so, int out_depth,
                         int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (!ct || !out || !ws) return fail(HEGPU_E_INVALID, "ckks_mod_raise: null argument");
    if (batch < 1) return fail(HEGPU_E_INVALID, "ckks_mod_raise: batch must be at least 1"); // (no grid limit here)
    if (out_depth < 0 || out_depth >= ctx->c.Q_size) return fail(HEGPU_E_INVALID, "ckks_mod_raise: 0 <= out_depth < Q");
    const Span in{ct, cs, ct_words(ctx->c, 1)}, res{out, so, level_words(ctx->c, out_depth)};
    const size_t need = ops_workspace_elems(ctx->c, OP_CKKS_MOD_RAISE, out_depth, batch) * sizeof(u64);
    if (int r = check_workspace(ws, ws_bytes, need)) return r;
    if (overlaps_any(res, {in}, batch)) return fail(HEGPU_E_INVALID, "ckks_mod_raise: out must not overlap ct");
    if (overlaps_any({(const uint64_t*) ws, 0, need / sizeof(u64)}, {res, in}, batch))
        return fail(HEGPU_E_INVALID, "ckks_mod_raise: the workspace must overlap neither out nor ct");
    NEED_CTX(ctx);
    return hip_ret(op_ckks_mod_raise(ctx->c, (const u64*) ct, cs, (u64*) out, so, out_depth, batch, (u64*) ws,
                                     (hipStream_t) stream),
                   "hegpu_ckks_mod_raise");
}

int hegpu_ckks_rotate_hoisted(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                              const uint64_t* const* keys, const int* galois_elts, int count, int depth, int batch,
                              void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, OP_CKKS_GALOIS, depth, batch, ws, ws_bytes)) return leave(r);
    if (count <= 0 || !keys || !galois_elts) return fail(HEGPU_E_INVALID, "rotate_hoisted: empty element list");
    const uint64_t words = level_words(ctx->c, depth);
    if (batch > 1 && so < (uint64_t) count * words) return fail(HEGPU_E_INVALID, "rotate_hoisted: out_stride too small");
    if (spans_overlap(ct, cs, words, out, so, (uint64_t) count * words, batch))
        return fail(HEGPU_E_INVALID, "rotate_hoisted: out must not alias ct (the result buffer must not contain the input)");
    if (int r = check_galois_list(ctx->c, keys, galois_elts, count, "rotate_hoisted")) return r;
    // with room for four accumulators (HEGPU_OP_CKKS_ROTATE_HOISTED) the inner products of four elements share one
    // read of the digits
    const int group = (ctx->c.fused_moddown && ctx->c.ntt_galois)
                          ? ops_rotate_hoisted_accumulators(ctx->c, depth, batch, ws_bytes / sizeof(u64)) : 1;
    return hip_ret(op_ckks_rotate_hoisted(ctx->c, (const u64*) ct, cs, (u64*) out, so, (const u64* const*) keys,
                                          galois_elts, count, depth, batch, (u64*) ws, (hipStream_t) stream, group),
                   "hegpu_ckks_rotate_hoisted");
}

int hegpu_ckks_diag_mac(hegpu_context* ctx, const uint64_t* rot, uint64_t rot_stride, int n1, const uint64_t* diags,
                        int n_diag, const int* index, int n2, uint64_t* out, uint64_t out_stride, int depth, int batch,
                        hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    if (!bsgs_shape_ok(n1, n2))
        return fail(HEGPU_E_INVALID, "diag_mac: n1 and n2 lie in [1, 16] (16 products per 128-bit sum, 256 indices by value)");
    if (!rot || !diags || !index || !out || n_diag < 1) return fail(HEGPU_E_INVALID, "diag_mac: null argument");
    if (int r = check_diag_index(index, n1, n2, n_diag, "diag_mac")) return r;
    if (int r = check_grid(batch, 1, "diag_mac")) return r;
    const uint64_t words = level_words(ctx->c, depth);
    if (spans_overlap(rot, rot_stride, (uint64_t) n1 * words, out, out_stride, (uint64_t) n2 * words, batch))
        return fail(HEGPU_E_INVALID, "diag_mac: out must not overlap rot");
    return hip_ret(rns_ckks_diag_mac((const u64*) rot, rot_stride, n1, (const u64*) diags, n_diag, index, n2, (u64*) out,
                                     out_stride, ctx->c.plan_qp.mods, ctx->c.n_power, ctx->c.Q_size - depth, batch,
                                     (hipStream_t) stream),
                   "hegpu_ckks_diag_mac");
}

size_t hegpu_ckks_linear_transform_workspace_bytes(const hegpu_context* ctx, int n1, int n2, int depth, int batch)
{
    if (!ctx || batch <= 0 || !bsgs_shape_ok(n1, n2) || depth < 0 || depth >= ctx->c.Q_size) return 0;
    return ops_linear_transform_workspace_elems(ctx->c, n1, n2, depth, batch) * sizeof(u64);
}

int hegpu_ckks_linear_transform(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                                const uint64_t* diags, int n_diag, const int* index, int n1, int n2,
                                const uint64_t* const* baby_keys, const int* baby_elts,
                                const uint64_t* const* giant_keys, const int* giant_elts, int depth, int batch, void* ws,
                                size_t ws_bytes, hegpu_stream stream)
{
    return hegpu_ckks_linear_transform_chained(ctx, ct, cs, out, so, diags, n_diag, index, n1, n2, baby_keys, baby_elts,
                                               giant_keys, giant_elts, nullptr, depth, batch, ws, ws_bytes, stream);
}

int hegpu_ckks_linear_transform_chained(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                                        const uint64_t* diags, int n_diag, const int* index, int n1, int n2,
                                        const uint64_t* const* baby_keys, const int* baby_elts,
                                        const uint64_t* const* giant_keys, const int* giant_elts, const int* giant_parent,
                                        int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    if (!bsgs_shape_ok(n1, n2)) return fail(HEGPU_E_INVALID, "linear_transform: n1 and n2 lie in [1, 16]");
    if (!ct || !out || !diags || !index || !baby_keys || !baby_elts || !giant_keys || !giant_elts || n_diag < 1)
        return fail(HEGPU_E_INVALID, "linear_transform: null argument");
    if (int r = check_diag_index(index, n1, n2, n_diag, "linear_transform")) return r;
    if (int r = check_grid(batch, 2, "linear_transform")) return r;
    if (int r = check_galois_list(ctx->c, baby_keys, baby_elts, n1, "linear_transform")) return r;
    if (int r = check_galois_list(ctx->c, giant_keys, giant_elts, n2, "linear_transform")) return r;
    if (int r = check_giant_chain(giant_parent, n2, giant_keys, giant_elts, "linear_transform")) return r;
    const uint64_t words = level_words(ctx->c, depth);
    if (spans_overlap(ct, cs, words, out, so, words, batch))
        return fail(HEGPU_E_INVALID, "linear_transform: out must not overlap ct");
    if (int r = check_workspace(ws, ws_bytes, hegpu_ckks_linear_transform_workspace_bytes(ctx, n1, n2, depth, batch)))
        return r;
    return hip_ret(op_ckks_linear_transform(ctx->c, (const u64*) ct, cs, (u64*) out, so, (const u64*) diags, n_diag, index,
                                            n1, n2, (const u64* const*) baby_keys, baby_elts,
                                            (const u64* const*) giant_keys, giant_elts, depth, batch, (u64*) ws,
                                            (hipStream_t) stream, giant_parent),
                   "hegpu_ckks_linear_transform");
}

// ---- polynomial evaluation: the two one-pass kernels and the sequence over a plan
int hegpu_ckks_weighted_sum(hegpu_context* ctx, const uint64_t* const* terms, const uint64_t* term_strides,
                            const int* term_limbs, const double* weights, int count, double w0_re, double w0_im,
                            uint64_t* out, uint64_t out_stride, int limbs, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_items(batch, 2, "weighted_sum")) return r;
    if (count < 0 || count > 15)
        return fail(HEGPU_E_INVALID, "weighted_sum: at most 15 terms (15 products and a residue per 128-bit sum)");
    if (limbs < 1 || limbs > ctx->c.Q_size) return fail(HEGPU_E_INVALID, "weighted_sum: bad limb count");
    if (!out || (count && (!terms || !term_strides || !term_limbs || !weights)))
        return fail(HEGPU_E_INVALID, "weighted_sum: null argument");
    for (double v : {w0_re, w0_im})
        if (!std::isfinite(v)) return fail(HEGPU_E_INVALID, "weighted_sum: a weight is not a finite number");
    const Span res{out, out_stride, ct_words(ctx->c, limbs)};
    for (int k = 0; k < count; k++) {
        if (!terms[k]) return fail(HEGPU_E_INVALID, "weighted_sum: null argument");
        if (term_limbs[k] < limbs || term_limbs[k] > ctx->c.Q_size)
            return fail(HEGPU_E_INVALID, "weighted_sum: a term has fewer limbs than the sum");
        if (!std::isfinite(weights[2 * k]) || !std::isfinite(weights[2 * k + 1]))
            return fail(HEGPU_E_INVALID, "weighted_sum: a weight is not a finite number");
        if (overlaps_any(res, {{terms[k], term_strides[k], ct_words(ctx->c, term_limbs[k])}}, batch))
            return fail(HEGPU_E_INVALID, "weighted_sum: out must not overlap a term");
    }
    return hip_ret(rns_ckks_weighted_sum((const u64* const*) terms, (const u64*) term_strides, term_limbs, weights, count,
                                         w0_re, w0_im, (u64*) out, out_stride, ctx->c.tab.psi_half, ctx->c.plan_qp.mods,
                                         ctx->c.n_power, limbs, batch, (hipStream_t) stream),
                   "hegpu_ckks_weighted_sum");
}

int hegpu_ckks_double_sub(hegpu_context* ctx, const uint64_t* a, uint64_t a_stride, int a_limbs, const uint64_t* b,
                          uint64_t b_stride, int b_limbs, double value, uint64_t* out, uint64_t out_stride, int limbs,
                          int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_items(batch, 2, "double_sub")) return r;
    if (!a || !out) return fail(HEGPU_E_INVALID, "double_sub: null argument");
    if (limbs < 1 || a_limbs < limbs || a_limbs > ctx->c.Q_size || (b && (b_limbs < limbs || b_limbs > ctx->c.Q_size)))
        return fail(HEGPU_E_INVALID, "double_sub: bad limb count");
    if (!b && !constant_in_range(value)) return fail(HEGPU_E_INVALID, "double_sub: constant out of range");
    const Span res{out, out_stride, ct_words(ctx->c, limbs)};
    const bool in_place = a == out && a_stride == out_stride && a_limbs == limbs;
    if (!in_place && overlaps_any(res, {{a, a_stride, ct_words(ctx->c, a_limbs)}}, batch))
        return fail(HEGPU_E_INVALID, "double_sub: out is a itself (equal strides and limb counts) or does not overlap it");
    if (b && overlaps_any(res, {{b, b_stride, ct_words(ctx->c, b_limbs)}}, batch))
        return fail(HEGPU_E_INVALID, "double_sub: out must not overlap b");
    return hip_ret(rns_ckks_double_sub((const u64*) a, a_stride, a_limbs, (const u64*) b, b_stride, b_limbs, value, (u64*) out,
                                       out_stride, ctx->c.plan_qp.mods, ctx->c.n_power, limbs, batch, (hipStream_t) stream),
                   "hegpu_ckks_double_sub");
}

size_t hegpu_ckks_poly_eval_workspace_bytes(const hegpu_context* ctx, const hegpu_poly_step* plan, int n_steps, int depth,
                                            int batch)
{
    if (!ctx || batch <= 0 || ctx->c.scheme != SCHEME_CKKS) return 0;
    size_t bytes = 0;
    (void) guarded([&]() -> int { // no exception may cross the C boundary (the check keeps tables of n_steps entries)
        if (!ops_poly_eval_check(ctx->c, plan, n_steps, depth))
            bytes = ops_poly_eval_workspace_elems(ctx->c, plan, n_steps, depth, batch) * sizeof(u64);
        return 0;
    });
    return bytes;
}

int hegpu_ckks_poly_eval(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                         const hegpu_poly_step* plan, int n_steps, const uint64_t* relin_key, int depth, int batch,
                         void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_items(batch, 2, "poly_eval")) return r;
    if (!ct || !out || !plan || !relin_key || !ws) return fail(HEGPU_E_INVALID, "poly_eval: null argument");
    return guarded([&]() -> int {
        if (const char* why = ops_poly_eval_check(ctx->c, plan, n_steps, depth))
            return fail(HEGPU_E_INVALID, std::string("poly_eval: ") + why);
        if (int r = check_leaf_weights(plan, n_steps, "poly_eval")) return r;
        const hegpu_poly_step& last = plan[n_steps - 1];
        const uint64_t out_words = ct_words(ctx->c, last.level + 1 + (last.rescale_after ? 1 : 0));
        if (spans_overlap(ct, cs, level_words(ctx->c, depth), out, so, out_words, batch))
            return fail(HEGPU_E_INVALID, "poly_eval: out must not overlap ct");
        if (int r = check_workspace(ws, ws_bytes, hegpu_ckks_poly_eval_workspace_bytes(ctx, plan, n_steps, depth, batch)))
            return r;
        return hip_ret(op_ckks_poly_eval(ctx->c, (const u64*) ct, cs, (u64*) out, so, plan, n_steps, (const u64*) relin_key, depth,
                                         batch, (u64*) ws, (hipStream_t) stream),
                       "hegpu_ckks_poly_eval");
    });
}

// ---- the real / imaginary boundary passes and the CoeffToSlot / SlotToCoeff sequences
static int conj_pass_check(const hegpu_context* ctx, int depth, int out_depth, int batch, const char* who)
{
    if (int r = check_items(batch, 2, who)) return r;
    return require(depth >= 0 && out_depth >= depth && out_depth < ctx->c.Q_size, std::string(who) + ": depth <= out_depth < Q");
}

int hegpu_ckks_conj_split(hegpu_context* ctx, const uint64_t* x, uint64_t x_stride, const uint64_t* xc,
                          uint64_t xc_stride, uint64_t* out0, uint64_t* out1, uint64_t out_stride, int depth,
                          int out_depth, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = conj_pass_check(ctx, depth, out_depth, batch, "conj_split")) return r;
    if (!x || !xc || !out0 || !out1) return fail(HEGPU_E_INVALID, "conj_split: null argument");
    const Span a{x, x_stride, level_words(ctx->c, depth)}, b{xc, xc == x ? x_stride : xc_stride, a.item}; // (sic: one buffer, x's stride)
    const Span res0{out0, out_stride, level_words(ctx->c, out_depth)}, res1{out1, out_stride, res0.item};
    if (overlaps_any(res0, {a, b}, batch) || overlaps_any(res1, {a, b}, batch))
        return fail(HEGPU_E_INVALID, "conj_split: an output must not overlap an input");
    if (overlaps_any(res1, {res0}, batch)) return fail(HEGPU_E_INVALID, "conj_split: the two outputs must not overlap");
    return hip_ret(rns_ckks_conj_split((const u64*) x, x_stride, (const u64*) xc, xc_stride, (u64*) out0, (u64*) out1,
                                       out_stride, ctx->c.tab.psi_half, ctx->c.plan_qp.mods, ctx->c.n_power,
                                       ctx->c.Q_size - depth, ctx->c.Q_size - out_depth, batch, (hipStream_t) stream),
                   "hegpu_ckks_conj_split");
}

int hegpu_ckks_conj_merge(hegpu_context* ctx, const uint64_t* c0, uint64_t c0_stride, const uint64_t* c1,
                          uint64_t c1_stride, uint64_t* out, uint64_t out_stride, int depth, int out_depth, int batch,
                          hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = conj_pass_check(ctx, depth, out_depth, batch, "conj_merge")) return r;
    if (!c0 || !c1 || !out) return fail(HEGPU_E_INVALID, "conj_merge: null argument");
    const uint64_t in_words = level_words(ctx->c, depth);
    if (overlaps_any({out, out_stride, level_words(ctx->c, out_depth)},
                     {{c0, c0_stride, in_words}, {c1, c1_stride, in_words}}, batch))
        return fail(HEGPU_E_INVALID, "conj_merge: the output must not overlap an input");
    return hip_ret(rns_ckks_conj_merge((const u64*) c0, c0_stride, (const u64*) c1, c1_stride, (u64*) out, out_stride,
                                       ctx->c.tab.psi_half, ctx->c.plan_qp.mods, ctx->c.n_power, ctx->c.Q_size - depth,
                                       ctx->c.Q_size - out_depth, batch, (hipStream_t) stream),
                   "hegpu_ckks_conj_merge");
}

// Everything is checked on the host tables, before the context is uploaded: a refusal needs no device.
int hegpu_ckks_conj_real(hegpu_context* ctx, const uint64_t* x, uint64_t x_stride, const uint64_t* xc, uint64_t xc_stride,
                         uint64_t* out, uint64_t out_stride, int depth, int out_depth, int batch, hegpu_stream stream)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = conj_pass_check(ctx, depth, out_depth, batch, "conj_real")) return r;
    if (!x || !xc || !out) return fail(HEGPU_E_INVALID, "conj_real: null argument");
    const Span a{x, x_stride, level_words(ctx->c, depth)}, b{xc, xc_stride, a.item}, res{out, out_stride, level_words(ctx->c, out_depth)};
    if (overlaps_any(res, {b}, batch)) return fail(HEGPU_E_INVALID, "conj_real: out must not overlap xc");
    const bool in_place = out == x && out_stride == x_stride && out_depth == depth;
    if (!in_place && overlaps_any(res, {a}, batch))
        return fail(HEGPU_E_INVALID, "conj_real: out is x itself (equal strides and depths) or does not overlap it");
    NEED_CTX(ctx);
    return hip_ret(rns_ckks_conj_real((const u64*) x, x_stride, (const u64*) xc, xc_stride, (u64*) out, out_stride,
                                      ctx->c.plan_qp.mods, ctx->c.n_power, ctx->c.Q_size - depth, ctx->c.Q_size - out_depth,
                                      batch, (hipStream_t) stream),
                   "hegpu_ckks_conj_real");
}

// the factor array of a sequence entry: every factor through the checks of hegpu_ckks_linear_transform's matrix arguments;
// boundary: the levels the sequence spends besides one per factor (the real / imaginary pass; the slim SlotToCoeff has none)
static int factors_check(const hegpu_context* ctx, const hegpu_linear_factor* f, int count, int depth, const char* who,
                         int boundary = 1)
{
    if (!f || count < 1) return fail(HEGPU_E_INVALID, std::string(who) + ": at least one factor");
    if (boundary == 0 && (depth < 0 || depth + count >= ctx->c.Q_size))
        return fail(HEGPU_E_INVALID, std::string(who) + ": depth + factors must stay below Q (one level per factor)");
    if (boundary != 0 && (depth < 0 || depth + count + 1 >= ctx->c.Q_size))
        return fail(HEGPU_E_INVALID, std::string(who) + ": depth + factors + 1 must stay below Q (one level per factor, one "
                                                        "at the real / imaginary boundary)");
    for (int k = 0; k < count; k++) {
        const hegpu_linear_factor& a = f[k];
        if (!bsgs_shape_ok(a.n1, a.n2)) return fail(HEGPU_E_INVALID, std::string(who) + ": n1 and n2 lie in [1, 16]");
        if (!a.diags || !a.index || !a.baby_keys || !a.baby_elts || !a.giant_keys || !a.giant_elts || a.n_diag < 1)
            return fail(HEGPU_E_INVALID, std::string(who) + ": null argument in a factor");
        if (int r = check_diag_index(a.index, a.n1, a.n2, a.n_diag, who)) return r;
        if (int r = check_galois_list(ctx->c, a.baby_keys, a.baby_elts, a.n1, who)) return r;
        if (int r = check_galois_list(ctx->c, a.giant_keys, a.giant_elts, a.n2, who)) return r;
        if (int r = check_giant_chain(a.giant_parent, a.n2, a.giant_keys, a.giant_elts, who)) return r;
    }
    return 0;
}

static std::vector<LinearFactor> factors_of(const hegpu_linear_factor* f, int count)
{
    std::vector<LinearFactor> v((size_t) count);
    for (int k = 0; k < count; k++)
        v[(size_t) k] = LinearFactor{(const u64*) f[k].diags, f[k].n_diag, f[k].index, f[k].n1, f[k].n2,
                                     (const u64* const*) f[k].baby_keys, f[k].baby_elts,
                                     (const u64* const*) f[k].giant_keys, f[k].giant_elts, f[k].giant_parent};
    return v;
}

size_t hegpu_ckks_encoding_transform_workspace_bytes(const hegpu_context* ctx, const hegpu_linear_factor* factors,
                                                     int count, int depth, int batch)
{
    if (!ctx || !factors || batch <= 0 || count < 1 || depth < 0 || depth >= ctx->c.Q_size) return 0;
    for (int k = 0; k < count; k++)
        if (!bsgs_shape_ok(factors[k].n1, factors[k].n2)) return 0;
    return ops_encoding_transform_workspace_elems(ctx->c, factors_of(factors, count).data(), count, depth, batch) *
           sizeof(u64);
}

int hegpu_ckks_coeff_to_slot(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out0, uint64_t* out1,
                             uint64_t so, const hegpu_linear_factor* factors, int count, const uint64_t* conj_key,
                             int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    if (int r = factors_check(ctx, factors, count, depth, "coeff_to_slot")) return r;
    if (!ct || !out0 || !out1 || !conj_key) return fail(HEGPU_E_INVALID, "coeff_to_slot: null argument");
    if (int r = check_grid(batch, 2, "coeff_to_slot")) return r;
    const uint64_t out_words = level_words(ctx->c, depth + count + 1);
    const Span in{ct, cs, level_words(ctx->c, depth)}, res0{out0, so, out_words}, res1{out1, so, out_words};
    if (overlaps_any(res0, {in}, batch) || overlaps_any(res1, {in, res0}, batch))
        return fail(HEGPU_E_INVALID, "coeff_to_slot: the outputs must overlap neither ct nor each other");
    if (int r = check_workspace(ws, ws_bytes, hegpu_ckks_encoding_transform_workspace_bytes(ctx, factors, count, depth, batch)))
        return r;
    return guarded([&]() -> int {
        return hip_ret(op_ckks_coeff_to_slot(ctx->c, (const u64*) ct, cs, (u64*) out0, (u64*) out1, so,
                                             factors_of(factors, count).data(), count, (const u64*) conj_key, depth,
                                             batch, (u64*) ws, (hipStream_t) stream),
                       "hegpu_ckks_coeff_to_slot");
    });
}

int hegpu_ckks_slot_to_coeff(hegpu_context* ctx, const uint64_t* c0, uint64_t c0_stride, const uint64_t* c1,
                             uint64_t c1_stride, uint64_t* out, uint64_t so, const hegpu_linear_factor* factors,
                             int count, int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    if (int r = factors_check(ctx, factors, count, depth, "slot_to_coeff")) return r;
    if (!c0 || !c1 || !out) return fail(HEGPU_E_INVALID, "slot_to_coeff: null argument");
    if (int r = check_grid(batch, 2, "slot_to_coeff")) return r;
    const uint64_t in_words = level_words(ctx->c, depth);
    const uint64_t out_words = level_words(ctx->c, depth + count); // before the last rescale
    if (batch > 1 && so < out_words) return fail(HEGPU_E_INVALID, "slot_to_coeff: out_stride too small");
    if (overlaps_any({out, so, out_words}, {{c0, c0_stride, in_words}, {c1, c1_stride, in_words}}, batch))
        return fail(HEGPU_E_INVALID, "slot_to_coeff: out must not overlap an input");
    if (int r = check_workspace(ws, ws_bytes, hegpu_ckks_encoding_transform_workspace_bytes(ctx, factors, count, depth, batch)))
        return r;
    return guarded([&]() -> int {
        return hip_ret(op_ckks_slot_to_coeff(ctx->c, (const u64*) c0, c0_stride, (const u64*) c1, c1_stride, (u64*) out, so,
                                             factors_of(factors, count).data(), count, depth, batch, (u64*) ws,
                                             (hipStream_t) stream),
                       "hegpu_ckks_slot_to_coeff");
    });
}

// ---- the CKKS refresh and the slim family.  Everything is checked on the host tables, before the context is uploaded: a
// refusal needs no device.  The two entries share their checks.  A RefreshKind is what differs between them there, a
// Refresh the arguments they have in common.
extern "C++" {
template <typename Plan>
struct RefreshKind {
    const char* who; // the name in the messages
    const char* (*plan_check)(const Context&, const Plan&, const host::PolyStep*, int);
    int32_t Plan::*stc_start; // the level of SlotToCoeff's first factor
    int stc_boundary;         // factors_check's: the regular SlotToCoeff merges the two halves first, the slim one has one input
};
static const RefreshKind<hegpu_bootstrap_plan> REGULAR_REFRESH{"bootstrap", ops_bootstrap_check, &hegpu_bootstrap_plan::stc_level, 1};
static const RefreshKind<hegpu_slim_bootstrap_plan> SLIM_REFRESH{"slim_bootstrap", ops_slim_bootstrap_check,
                                                                 &hegpu_slim_bootstrap_plan::in_level, 0};
template <typename Plan>
struct Refresh {
    const RefreshKind<Plan>& kind;
    const hegpu_context* ctx;
    const Plan* plan;
    const hegpu_poly_step* steps; // the EvalMod or trig plan
    int n_steps;
    const hegpu_linear_factor *cts, *stc;
    int cts_count, stc_count, batch;
};

template <typename Plan>
static int refresh_check(const Refresh<Plan>& r)
{
    const std::string who = r.kind.who;
    if (!r.ctx) return fail(HEGPU_E_INVALID, "null context");
    if (int e = check_scheme(r.ctx->c, SCHEME_CKKS)) return e;
    if (!r.plan || !r.steps || !r.cts || !r.stc) return fail(HEGPU_E_INVALID, who + ": null argument");
    if (int e = check_items(r.batch, 4, r.kind.who)) return e;
    const Plan& p = *r.plan;
    if (const char* why = r.kind.plan_check(r.ctx->c, p, r.steps, r.n_steps)) return fail(HEGPU_E_INVALID, who + ": " + why);
    if (r.cts_count != p.cts_pieces || r.stc_count != p.stc_pieces)
        return fail(HEGPU_E_INVALID, who + ": as many factors as the plan has pieces");
    const int Q = r.ctx->c.Q_size;
    if (int e = factors_check(r.ctx, r.cts, p.cts_pieces, Q - 1 - p.cts_level, (who + " (CoeffToSlot)").c_str())) return e;
    return factors_check(r.ctx, r.stc, p.stc_pieces, Q - 1 - p.*r.kind.stc_start, (who + " (SlotToCoeff)").c_str(),
                         r.kind.stc_boundary);
}

// the size query: 0 for arguments the check refuses; elems(cts, stc): the words of the sequence for the checked ones
template <typename Plan, typename Elems>
static size_t refresh_workspace_bytes(const Refresh<Plan>& r, Elems&& elems)
{
    size_t bytes = 0;
    (void) guarded([&]() -> int { // no exception may cross the C boundary
        if (!refresh_check(r))
            bytes = elems(factors_of(r.cts, r.cts_count).data(), factors_of(r.stc, r.stc_count).data()) * sizeof(u64);
        return 0;
    });
    return bytes;
}

// What both entries do after refresh_check and the null check of their own arguments.  in, in2: the inputs (an entry with
// one passes it twice); res: the room `out` needs; need: the size query's answer; out_rule, ws_rule: the refusals of an
// overlap, which name the entry's inputs.
template <typename Plan, typename Launch>
static int refresh_run(const Refresh<Plan>& r, hegpu_context* ctx, const Span& in, const Span& in2, const Span& res, const void* ws,
                       size_t ws_bytes, size_t need, const char* out_rule, const char* ws_rule, Launch&& launch)
{
    const std::string who = r.kind.who;
    if (int e = check_leaf_weights(r.steps, r.n_steps, r.kind.who)) return e;
    if (r.batch > 1 && res.stride < res.item) return fail(HEGPU_E_INVALID, who + ": out_stride too small");
    if (!need || ws_bytes < need) return fail(HEGPU_E_INVALID, "workspace too small");
    if (overlaps_any(res, {in, in2}, r.batch)) return fail(HEGPU_E_INVALID, who + ": " + out_rule);
    if (overlaps_any({(const uint64_t*) ws, 0, need / sizeof(u64)}, {res, in, in2}, r.batch))
        return fail(HEGPU_E_INVALID, who + ": " + ws_rule);
    NEED_CTX(ctx);
    return launch();
}
} // extern "C++"

size_t hegpu_ckks_bootstrap_workspace_bytes(const hegpu_context* ctx, const hegpu_bootstrap_plan* plan,
                                            const hegpu_poly_step* eval_mod, int n_steps, const hegpu_linear_factor* cts,
                                            int cts_count, const hegpu_linear_factor* stc, int stc_count, int switch_keys,
                                            int batch)
{
    const Refresh<hegpu_bootstrap_plan> r{REGULAR_REFRESH, ctx, plan, eval_mod, n_steps, cts, stc, cts_count, stc_count, batch};
    return refresh_workspace_bytes(r, [&](const LinearFactor* c, const LinearFactor* s) {
        return ops_bootstrap_workspace_elems(ctx->c, *plan, eval_mod, n_steps, c, s, switch_keys != 0, batch);
    });
}

int hegpu_ckks_bootstrap(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                         const hegpu_bootstrap_plan* plan, const hegpu_poly_step* eval_mod, int n_steps,
                         const hegpu_linear_factor* cts, int cts_count, const hegpu_linear_factor* stc, int stc_count,
                         const uint64_t* conj_key, const uint64_t* relin_key, const uint64_t* swk_dense_to_sparse, const uint64_t* swk_sparse_to_dense,
                         int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return guarded([&]() -> int {
        const Refresh<hegpu_bootstrap_plan> r{REGULAR_REFRESH, ctx, plan, eval_mod, n_steps, cts, stc, cts_count, stc_count, batch};
        if (int e = refresh_check(r)) return e;
        if (!ct || !out || !conj_key || !relin_key || !ws) return fail(HEGPU_E_INVALID, "bootstrap: null argument");
        if (!swk_dense_to_sparse != !swk_sparse_to_dense)
            return fail(HEGPU_E_INVALID, "bootstrap: both switch keys (dense to sparse, sparse to dense) or neither");
        const Span in{ct, cs, ct_words(ctx->c, 1)}, res{out, so, ct_words(ctx->c, plan->out_level + 2)}; // before the last rescale
        const size_t need = hegpu_ckks_bootstrap_workspace_bytes(ctx, plan, eval_mod, n_steps, cts, cts_count, stc, stc_count,
                                                                 swk_dense_to_sparse != nullptr, batch);
        return refresh_run(r, ctx, in, in, res, ws, ws_bytes, need, "out must not overlap ct",
                           "the workspace must overlap neither out nor ct", [&]() -> int {
            return hip_ret(op_ckks_bootstrap(ctx->c, (const u64*) ct, cs, (u64*) out, so, *plan, eval_mod, n_steps,
                                             factors_of(cts, cts_count).data(), factors_of(stc, stc_count).data(),
                                             (const u64*) conj_key, (const u64*) relin_key, (const u64*) swk_dense_to_sparse,
                                             (const u64*) swk_sparse_to_dense, batch, (u64*) ws, (hipStream_t) stream),
                           "hegpu_ckks_bootstrap");
        });
    });
}

size_t hegpu_ckks_slim_bootstrap_workspace_bytes(const hegpu_context* ctx, const hegpu_slim_bootstrap_plan* plan,
                                                 const hegpu_poly_step* trig, int n_steps, const hegpu_linear_factor* cts,
                                                 int cts_count, const hegpu_linear_factor* stc, int stc_count, int batch)
{
    const Refresh<hegpu_slim_bootstrap_plan> r{SLIM_REFRESH, ctx, plan, trig, n_steps, cts, stc, cts_count, stc_count, batch};
    return refresh_workspace_bytes(r, [&](const LinearFactor* c, const LinearFactor* s) {
        return ops_slim_bootstrap_workspace_elems(ctx->c, *plan, trig, n_steps, c, s, batch);
    });
}

int hegpu_ckks_slim_bootstrap(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, const uint64_t* ct2, uint64_t cs2,
                              uint64_t* out, uint64_t so, const hegpu_slim_bootstrap_plan* plan, const hegpu_poly_step* trig,
                              int n_steps, const hegpu_linear_factor* cts, int cts_count, const hegpu_linear_factor* stc,
                              int stc_count, const uint64_t* conj_key, const uint64_t* relin_key, int batch, void* ws,
                              size_t ws_bytes, hegpu_stream stream)
{
    return guarded([&]() -> int {
        const Refresh<hegpu_slim_bootstrap_plan> r{SLIM_REFRESH, ctx, plan, trig, n_steps, cts, stc, cts_count, stc_count, batch};
        if (int e = refresh_check(r)) return e;
        if (!ct || !out || !conj_key || !relin_key || !ws) return fail(HEGPU_E_INVALID, "slim_bootstrap: null argument");
        const uint64_t in_words = ct_words(ctx->c, plan->in_level + 1);
        const Span in{ct, cs, in_words}, in2{ct2 ? ct2 : ct, ct2 ? cs2 : cs, in_words};
        const Span res{out, so, ct_words(ctx->c, plan->out_level + 1 + (trig[n_steps - 1].rescale_after ? 1 : 0))};
        const size_t need = hegpu_ckks_slim_bootstrap_workspace_bytes(ctx, plan, trig, n_steps, cts, cts_count, stc, stc_count, batch);
        return refresh_run(r, ctx, in, in2, res, ws, ws_bytes, need, "out must overlap neither ct nor ct2",
                           "the workspace must overlap neither out nor ct nor ct2", [&]() -> int {
            return hip_ret(op_ckks_slim_bootstrap(ctx->c, (const u64*) ct, cs, (const u64*) ct2, cs2, (u64*) out, so, *plan, trig,
                                                  n_steps, factors_of(cts, cts_count).data(), factors_of(stc, stc_count).data(),
                                                  (const u64*) conj_key, (const u64*) relin_key, batch, (u64*) ws,
                                                  (hipStream_t) stream),
                           "hegpu_ckks_slim_bootstrap");
        });
    });
}

int hegpu_bfv_multiply(hegpu_context* ctx, const uint64_t* ct1, uint64_t s1, const uint64_t* ct2, uint64_t s2,
                       uint64_t* out, uint64_t so, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (int r = check_batch(batch)) return leave(r);
    if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_BFV_MULTIPLY, 0, batch))) return r;
    return hip_ret(op_bfv_multiply(ctx->c, (const u64*) ct1, s1, (const u64*) ct2, s2, (u64*) out, so, batch,
                                   (u64*) ws, (hipStream_t) stream),
                   "hegpu_bfv_multiply");
}

int hegpu_bfv_relinearize_inplace(hegpu_context* ctx, uint64_t* ct, uint64_t cs, const uint64_t* key, int batch,
                                  void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_BFV, OP_BFV_RELIN, 0, batch, ws, ws_bytes)) return leave(r);
    return hip_ret(op_bfv_relinearize(ctx->c, (u64*) ct, cs, (const u64*) key, batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_bfv_relinearize_inplace");
}

int hegpu_bfv_apply_galois(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t* out, uint64_t so,
                           const uint64_t* key, int galois_elt, int batch, void* ws, size_t ws_bytes,
                           hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_BFV, OP_BFV_GALOIS, 0, batch, ws, ws_bytes)) return leave(r);
    const uint64_t words = level_words(ctx->c, 0);
    if (spans_overlap(ct, cs, words, out, so, words, batch))
        return fail(HEGPU_E_INVALID, "apply_galois: out must not alias ct (the result buffer must not contain the input)");
    return hip_ret(op_bfv_apply_galois(ctx->c, (const u64*) ct, cs, (u64*) out, so, (const u64*) key, galois_elt, batch,
                                       (u64*) ws, (hipStream_t) stream),
                   "hegpu_bfv_apply_galois");
}

// ------------------------------------------------------------------ key generation / encryption / decryption
struct hegpu_rng {
    Rng r;
};

int hegpu_rng_create(uint64_t seed, hegpu_rng** out)
{
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("null output");
        hegpu_rng* h = new hegpu_rng();
        h->r.seed = drbg_key_from_u64(seed);
        *out = h;
        return 0;
    });
}

int hegpu_rng_create_seeded(const uint8_t seed[32], hegpu_rng** out)
{
    return guarded([&]() -> int {
        if (!out || !seed) throw std::invalid_argument("null argument");
        hegpu_rng* h = new hegpu_rng();
        for (int i = 0; i < 8; i++)
            h->r.seed.k[i] = (u32) seed[4 * i] | ((u32) seed[4 * i + 1] << 8) | ((u32) seed[4 * i + 2] << 16) |
                             ((u32) seed[4 * i + 3] << 24);
        *out = h;
        return 0;
    });
}

int hegpu_rng_create_from_entropy(hegpu_rng** out)
{
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("null output");
        uint8_t seed[32];
        size_t got = 0;
        while (got < sizeof(seed)) {
            const ssize_t r = getrandom(seed + got, sizeof(seed) - got, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                throw std::runtime_error("getrandom failed: no entropy source for the key generator");
            }
            got += (size_t) r;
        }
        const int rc = hegpu_rng_create_seeded(seed, out);
        volatile uint8_t* z = seed;
        for (size_t i = 0; i < sizeof(seed); i++) z[i] = 0;
        return rc;
    });
}

int hegpu_drbg_block(const uint8_t key[32], uint64_t stream, uint64_t index, uint32_t out[4])
{
    if (!key || !out) return fail(HEGPU_E_INVALID, "null argument");
    DrbgKey k;
    for (int i = 0; i < 8; i++)
        k.k[i] = (u32) key[4 * i] | ((u32) key[4 * i + 1] << 8) | ((u32) key[4 * i + 2] << 16) | ((u32) key[4 * i + 3] << 24);
    const DrbgOut o = drbg_block(k, stream, index);
    for (int i = 0; i < 4; i++) out[i] = o.w[i];
    return 0;
}

void hegpu_rng_destroy(hegpu_rng* rng)
{
    if (!rng) return;
    explicit_bzero(&rng->r, sizeof(rng->r)); // the 256-bit key must not stay behind in freed heap memory
    delete rng;
}

// key generation and encryption: the party's generator and the workspace row `op` for one item
static int check_kg(const hegpu_context* ctx, const hegpu_rng* rng, int op, const void* ws, size_t ws_bytes)
{
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    return check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, op, 0, 1));
}

int hegpu_generate_secret_key(hegpu_context* ctx, hegpu_rng* rng, int hamming_weight, uint64_t* sk, void* ws,
                              size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_generate_secret_key", SYNCS)) return r; // (and it draws)
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_KEYGEN_SECRET, ws, ws_bytes)) return r;
    if (hamming_weight <= 0 || hamming_weight > (int) ctx->c.n)
        return fail(HEGPU_E_INVALID, "hamming weight has to be in range 0 to ring size"); // secretkey.cu:43
    return hip_ret(op_gen_secret_key(ctx->c, rng->r, hamming_weight, (u64*) sk, (u64*) ws, (hipStream_t) stream),
                   "hegpu_generate_secret_key");
}

int hegpu_generate_public_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, uint64_t* pk, void* ws,
                              size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_generate_public_key", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_KEYGEN_PUBLIC, ws, ws_bytes)) return r;
    return hip_ret(op_gen_public_key(ctx->c, rng->r, (const u64*) sk, (u64*) pk, (u64*) ws, (hipStream_t) stream),
                   "hegpu_generate_public_key");
}

int hegpu_generate_relin_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, uint64_t* rk, void* ws,
                             size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_generate_relin_key", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_KEYGEN_SWITCH, ws, ws_bytes)) return r;
    return hip_ret(op_gen_switch_key(ctx->c, rng->r, (const u64*) sk, 0, nullptr, (u64*) rk, (u64*) ws,
                                     (hipStream_t) stream),
                   "hegpu_generate_relin_key");
}

int hegpu_generate_switch_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* new_sk, const uint64_t* old_sk,
                              uint64_t* swk, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_generate_switch_key", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_KEYGEN_SWITCH, ws, ws_bytes)) return r;
    if (!old_sk) return fail(HEGPU_E_INVALID, "null old secret key");
    return hip_ret(op_gen_switch_key(ctx->c, rng->r, (const u64*) new_sk, 0, (const u64*) old_sk, (u64*) swk, (u64*) ws,
                                     (hipStream_t) stream),
                   "hegpu_generate_switch_key");
}

int hegpu_generate_galois_key(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, int galois_elt, uint64_t* gk,
                              void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_generate_galois_key", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_KEYGEN_SWITCH, ws, ws_bytes)) return r;
    if (!galois_elt_ok(ctx->c, galois_elt)) return fail(HEGPU_E_INVALID, "galois element must be odd and below 2N");
    return hip_ret(op_gen_switch_key(ctx->c, rng->r, (const u64*) sk, galois_elt, nullptr, (u64*) gk, (u64*) ws,
                                     (hipStream_t) stream),
                   "hegpu_generate_galois_key");
}

int hegpu_ckks_encrypt(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* pk, const uint64_t* plain, uint64_t* ct,
                       void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_ckks_encrypt", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_kg(ctx, rng, OP_CKKS_ENCRYPT, ws, ws_bytes)) return r;
    return hip_ret(op_ckks_encrypt(ctx->c, rng->r, (const u64*) pk, (const u64*) plain, (u64*) ct, (u64*) ws,
                                   (hipStream_t) stream),
                   "hegpu_ckks_encrypt");
}

int hegpu_ckks_decrypt(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, int depth, uint64_t* plain,
                       hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_depth(ctx->c, depth)) return r;
    return hip_ret(op_ckks_decrypt(ctx->c, (const u64*) ct, (const u64*) sk, depth, (u64*) plain,
                                   (hipStream_t) stream),
                   "hegpu_ckks_decrypt");
}

int hegpu_bfv_encrypt(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* pk, const uint64_t* plain, uint64_t* ct,
                      void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_bfv_encrypt", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (int r = check_kg(ctx, rng, OP_BFV_ENCRYPT, ws, ws_bytes)) return r;
    return hip_ret(op_bfv_encrypt(ctx->c, rng->r, (const u64*) pk, (const u64*) plain, (u64*) ct, (u64*) ws,
                                  (hipStream_t) stream),
                   "hegpu_bfv_encrypt");
}

int hegpu_bfv_decrypt(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, uint64_t* plain, void* ws,
                      size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_BFV_DECRYPT, 0, 1))) return r;
    return guarded([&]() -> int {
        return hip_ret(op_bfv_decrypt(ctx->c, (const u64*) ct, (const u64*) sk, (u64*) plain, (u64*) ws,
                                      (hipStream_t) stream),
                       "hegpu_bfv_decrypt");
    });
}

// ------------------------------------------------------------------ N-out-of-N multiparty protocol
static int check_mpc_kg(const hegpu_context* ctx, const hegpu_rng* crs, const hegpu_rng* rng, const void* ws, size_t ws_bytes)
{
    if (int r = check_kg(ctx, rng, OP_MPC_KEY_SHARE, ws, ws_bytes)) return r;
    if (!crs) return fail(HEGPU_E_INVALID, "null common random generator");
    return require(crs != rng, "crs and rng must be different generators: the party's errors are private");
}

static int check_shares(const uint64_t* const* shares, int k, const void* out)
{
    if (!shares || k < 1) return fail(HEGPU_E_INVALID, "at least one share is needed");
    for (int i = 0; i < k; i++) {
        if (!shares[i]) return fail(HEGPU_E_INVALID, "null share");
        if (shares[i] == out) return fail(HEGPU_E_INVALID, "the result must not be one of the shares");
    }
    return 0;
}

int hegpu_mpc_public_key_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk, uint64_t* share,
                               void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_public_key_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_mpc_kg(ctx, crs, rng, ws, ws_bytes)) return r;
    if (!sk || !share) return fail(HEGPU_E_INVALID, "null argument");
    return hip_ret(op_mpc_public_key_share(ctx->c, crs->r, rng->r, (const u64*) sk, (u64*) share, (u64*) ws,
                                           (hipStream_t) stream),
                   "hegpu_mpc_public_key_share");
}

int hegpu_mpc_relin_key_share_round1(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk,
                                     uint64_t* u_out, uint64_t* share, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_relin_key_share_round1", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_mpc_kg(ctx, crs, rng, ws, ws_bytes)) return r;
    if (!sk || !share || !u_out) return fail(HEGPU_E_INVALID, "null argument");
    return hip_ret(op_mpc_switch_key_share(ctx->c, crs->r, rng->r, (const u64*) sk, 0, (u64*) u_out, (u64*) share,
                                           (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_relin_key_share_round1");
}

int hegpu_mpc_relin_key_share_round2(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* sk, const uint64_t* u,
                                     const uint64_t* round1_sum, uint64_t* share, void* ws, size_t ws_bytes,
                                     hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_relin_key_share_round2", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_kg(ctx, rng, OP_MPC_KEY_SHARE, ws, ws_bytes)) return r;
    if (!sk || !u || !round1_sum || !share) return fail(HEGPU_E_INVALID, "null argument");
    if (share == round1_sum) return fail(HEGPU_E_INVALID, "the share must not overwrite the round-1 sum");
    return hip_ret(op_mpc_relin_key_share_round2(ctx->c, rng->r, (const u64*) sk, (const u64*) u,
                                                 (const u64*) round1_sum, (u64*) share, (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_relin_key_share_round2");
}

int hegpu_mpc_galois_key_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* sk, int galois_elt,
                               uint64_t* share, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_galois_key_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_mpc_kg(ctx, crs, rng, ws, ws_bytes)) return r;
    if (!sk || !share) return fail(HEGPU_E_INVALID, "null argument");
    if (!galois_elt_ok(ctx->c, galois_elt)) return fail(HEGPU_E_INVALID, "galois element must be odd and below 2N");
    return hip_ret(op_mpc_switch_key_share(ctx->c, crs->r, rng->r, (const u64*) sk, galois_elt, nullptr, (u64*) share,
                                           (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_galois_key_share");
}

int hegpu_mpc_accumulate(hegpu_context* ctx, const uint64_t* const* shares, int k, int layout, uint64_t* out,
                         hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (!out) return fail(HEGPU_E_INVALID, "null argument");
    if (layout != HEGPU_MPC_PUBLIC_KEY && layout != HEGPU_MPC_GALOIS_KEY && layout != HEGPU_MPC_RELIN_ROUND1)
        return fail(HEGPU_E_INVALID, "unknown share layout");
    if (const int rc = check_shares(shares, k, out)) return rc;
    return hip_ret(op_mpc_accumulate(ctx->c, (const u64* const*) shares, k, layout, nullptr, (u64*) out,
                                     (hipStream_t) stream),
                   "hegpu_mpc_accumulate");
}

int hegpu_mpc_relin_key_finish(hegpu_context* ctx, const uint64_t* const* round2_shares, int k,
                               const uint64_t* round1_sum, uint64_t* rk, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (!rk || !round1_sum) return fail(HEGPU_E_INVALID, "null argument");
    if (rk == round1_sum) return fail(HEGPU_E_INVALID, "the key must not overwrite the round-1 sum");
    if (const int rc = check_shares(round2_shares, k, rk)) return rc;
    return hip_ret(op_mpc_accumulate(ctx->c, (const u64* const*) round2_shares, k, MPC_LAYOUT_RELIN_FINISH,
                                     (const u64*) round1_sum, (u64*) rk, (hipStream_t) stream),
                   "hegpu_mpc_relin_key_finish");
}

int hegpu_mpc_ckks_decrypt_share(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* ct, uint64_t cs,
                                 const uint64_t* sk, int depth, uint64_t* share, int batch, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_ckks_decrypt_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    if (!ct || !sk || !share) return fail(HEGPU_E_INVALID, "null argument");
    return hip_ret(op_mpc_ckks_decrypt_share(ctx->c, rng->r, (const u64*) ct, cs, (const u64*) sk, depth, (u64*) share,
                                             batch, (hipStream_t) stream),
                   "hegpu_mpc_ckks_decrypt_share");
}

int hegpu_mpc_ckks_decrypt_merge(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, const uint64_t* const* shares,
                                 int k, int depth, uint64_t* plain, int batch, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (!ct || !plain) return fail(HEGPU_E_INVALID, "null argument");
    if (const int rc = check_shares(shares, k, plain)) return rc;
    if (int r = check_op(ctx, SCHEME_CKKS, 0, depth, batch, nullptr, 0)) return leave(r);
    return hip_ret(op_mpc_ckks_decrypt_merge(ctx->c, (const u64*) ct, cs, (const u64* const*) shares, k, depth,
                                             (u64*) plain, batch, (hipStream_t) stream),
                   "hegpu_mpc_ckks_decrypt_merge");
}

int hegpu_mpc_bfv_decrypt_share(hegpu_context* ctx, hegpu_rng* rng, const uint64_t* ct, uint64_t cs,
                                const uint64_t* sk, uint64_t* share, int batch, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_bfv_decrypt_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = check_op(ctx, SCHEME_BFV, 0, 0, batch, nullptr, 0)) return leave(r);
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    if (!ct || !sk || !share) return fail(HEGPU_E_INVALID, "null argument");
    return hip_ret(op_mpc_bfv_decrypt_share(ctx->c, rng->r, (const u64*) ct, cs, (const u64*) sk, (u64*) share, batch,
                                            (hipStream_t) stream),
                   "hegpu_mpc_bfv_decrypt_share");
}

int hegpu_mpc_bfv_decrypt_merge(hegpu_context* ctx, const uint64_t* ct, uint64_t cs, const uint64_t* const* shares,
                                int k, uint64_t* plain, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (!ct || !plain) return fail(HEGPU_E_INVALID, "null argument");
    if (const int rc = check_shares(shares, k, plain)) return rc;
    if (int r = check_op(ctx, SCHEME_BFV, OP_MPC_BFV_DECRYPT_MERGE, 0, batch, ws, ws_bytes)) return leave(r);
    return hip_ret(op_mpc_bfv_decrypt_merge(ctx->c, (const u64*) ct, cs, (const u64* const*) shares, k, (u64*) plain,
                                            batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_bfv_decrypt_merge");
}

// ---- collective refresh.  The checks every entry shares; the workspace row may be empty (a share needs none)
// The two merges take the common generator only to derive the public a of the shares again; they draw nothing of their
// own and stay capturable.  A replay derives the a of the captured call: the shares of every replay must come from a
// common generator as far advanced as the one the capture was given.
// Unlike the operators, the depth and the common generator are looked at before an empty batch leaves.
static int check_refresh(const hegpu_context* ctx, int want_scheme, int op, int depth, int batch, const hegpu_rng* crs,
                         const void* ws, size_t ws_bytes)
{
    if (int r = check_scheme(ctx->c, want_scheme)) return r;
    const int b = check_batch(batch);
    if (b > 0) return b;
    if (int r = check_depth(ctx->c, depth)) return r;
    if (!crs) return fail(HEGPU_E_INVALID, "null common random generator");
    if (b) return b;
    const size_t need = hegpu_workspace_bytes(ctx, op, depth, batch);
    return need ? check_workspace(ws, ws_bytes, need) : 0;
}

static int check_refresh_party(const hegpu_rng* rng, const void* ct, const void* sk, const void* share)
{
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    return require(ct && sk && share, "null argument");
}

// out [batch] items of 2 Q N words, out_stride apart, must share no word with the input batch or with a share
static int check_refresh_out(const hegpu_context* ctx, const uint64_t* ct, uint64_t cs, uint64_t in_words,
                             const uint64_t* const* shares, int k, uint64_t share_words, const uint64_t* out,
                             uint64_t so, int batch)
{
    if (!ct || !out) return fail(HEGPU_E_INVALID, "null argument");
    if (const int rc = check_shares(shares, k, out)) return rc;
    const Span res{out, so, level_words(ctx->c, 0)};
    if (batch > 1 && (so < res.item || cs < in_words))
        return fail(HEGPU_E_INVALID, "the items of a batch overlap: stride below the size of an item");
    if (overlaps_any(res, {{ct, cs, in_words}}, batch))
        return fail(HEGPU_E_INVALID, "the result overlaps the input ciphertexts");
    for (int i = 0; i < k; i++)
        if (overlaps_any(res, {{shares[i], share_words, share_words}}, batch))
            return fail(HEGPU_E_INVALID, "the result overlaps a share");
    return 0;
}

int hegpu_mpc_ckks_refresh_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* ct, uint64_t cs,
                                 const uint64_t* sk, int depth, int mask_bits, uint64_t* share, int batch, void* ws,
                                 size_t ws_bytes, hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_ckks_refresh_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = require(!crs || crs != rng, "crs and rng must be different generators: the party's mask and errors are private"))
        return r;
    if (int r = check_refresh(ctx, SCHEME_CKKS, OP_MPC_REFRESH_SHARE, depth, batch, crs, ws, ws_bytes)) return leave(r);
    if (const int rc = check_refresh_party(rng, ct, sk, share)) return rc;
    // 2^mask_bits >= Q_level / 2 can never be unmasked, whatever the message and the number of parties
    if (mask_bits < 1 || mask_bits > 126 || mask_bits + 1 >= level_modulus_bits(ctx->c, ctx->c.Q_size - depth))
        return fail(HEGPU_E_INVALID, "mask_bits must be in [1, 126] with 2^mask_bits below half the level's modulus");
    return hip_ret(op_mpc_ckks_refresh_share(ctx->c, crs->r, rng->r, (const u64*) ct, cs, (const u64*) sk, depth,
                                             mask_bits, (u64*) share, batch, (hipStream_t) stream),
                   "hegpu_mpc_ckks_refresh_share");
}

int hegpu_mpc_ckks_refresh_merge(hegpu_context* ctx, hegpu_rng* crs, const uint64_t* ct, uint64_t cs,
                                 const uint64_t* const* shares, int k, int depth, uint64_t* out, uint64_t so, int batch,
                                 void* ws, size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_refresh(ctx, SCHEME_CKKS, OP_MPC_REFRESH_MERGE, depth, batch, crs, ws, ws_bytes)) return leave(r);
    const int l = ctx->c.Q_size - depth;
    const uint64_t share_words = ct_words(ctx->c, l + ctx->c.Q_size, 1);
    if (const int rc = check_refresh_out(ctx, ct, cs, ct_words(ctx->c, l), shares, k, share_words, out, so, batch)) return rc;
    return hip_ret(op_mpc_ckks_refresh_merge(ctx->c, crs->r, (const u64*) ct, cs, (const u64* const*) shares, k, depth,
                                             (u64*) out, so, batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_ckks_refresh_merge");
}

int hegpu_mpc_bfv_refresh_share(hegpu_context* ctx, hegpu_rng* crs, hegpu_rng* rng, const uint64_t* ct, uint64_t cs,
                                const uint64_t* sk, uint64_t* share, int batch, void* ws, size_t ws_bytes,
                                hegpu_stream stream)
{
    if (int r = check_not_capturing(stream, "hegpu_mpc_bfv_refresh_share", DRAWS)) return r;
    NEED_CTX(ctx);
    if (int r = require(!crs || crs != rng, "crs and rng must be different generators: the party's mask and errors are private"))
        return r;
    if (int r = check_refresh(ctx, SCHEME_BFV, OP_MPC_REFRESH_SHARE, 0, batch, crs, ws, ws_bytes)) return leave(r);
    if (const int rc = check_refresh_party(rng, ct, sk, share)) return rc;
    return hip_ret(op_mpc_bfv_refresh_share(ctx->c, crs->r, rng->r, (const u64*) ct, cs, (const u64*) sk, (u64*) share,
                                            batch, (hipStream_t) stream),
                   "hegpu_mpc_bfv_refresh_share");
}

int hegpu_mpc_bfv_refresh_merge(hegpu_context* ctx, hegpu_rng* crs, const uint64_t* ct, uint64_t cs,
                                const uint64_t* const* shares, int k, uint64_t* out, uint64_t so, int batch, void* ws,
                                size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_refresh(ctx, SCHEME_BFV, OP_MPC_REFRESH_MERGE, 0, batch, crs, ws, ws_bytes)) return leave(r);
    const uint64_t words = level_words(ctx->c, 0);
    if (const int rc = check_refresh_out(ctx, ct, cs, words, shares, k, words, out, so, batch)) return rc;
    return hip_ret(op_mpc_bfv_refresh_merge(ctx->c, crs->r, (const u64*) ct, cs, (const u64* const*) shares, k,
                                            (u64*) out, so, batch, (u64*) ws, (hipStream_t) stream),
                   "hegpu_mpc_bfv_refresh_merge");
}

int hegpu_bfv_encode(hegpu_context* ctx, const int64_t* message, int message_size, uint64_t* plain,
                     hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (!ctx->c.plan_plain.count)
        return fail(HEGPU_E_LOGIC, "batching needs a prime plain modulus with 2N | t - 1");
    if (message_size < 0 || message_size > (int) ctx->c.n)
        return fail(HEGPU_E_INVALID, "Message size can not be higher than the slot count."); // bfv/encoder.cuh:60
    if (!message && message_size > 0) return fail(HEGPU_E_INVALID, "message is null");
    return hip_ret(op_bfv_encode(ctx->c, (const long long*) message, message_size, (u64*) plain,
                                 (hipStream_t) stream),
                   "hegpu_bfv_encode");
}

int hegpu_bfv_decode(hegpu_context* ctx, const uint64_t* plain, uint64_t* message, void* ws, size_t ws_bytes,
                     hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (!ctx->c.plan_plain.count)
        return fail(HEGPU_E_LOGIC, "batching needs a prime plain modulus with 2N | t - 1");
    if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_BFV_DECODE, 0, 1))) return r;
    return hip_ret(op_bfv_decode(ctx->c, (const u64*) plain, (u64*) message, (u64*) ws, (hipStream_t) stream),
                   "hegpu_bfv_decode");
}

static int ckks_encode_any(hegpu_context* ctx, int mode, const double* message, int message_size, double scalar,
                           double scale, uint64_t* plain, void* ws, size_t ws_bytes, hegpu_stream stream, const char* who)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (mode == 2) {
        if (message_size < 0 || message_size > (int) ctx->c.n)
            return fail(HEGPU_E_INVALID, "Vector size can not be higher than polynomial degree!"); // ckks/encoder.cuh:80
    } else if (mode != 3 && (message_size < 0 || message_size > (int) (ctx->c.n >> 1))) {
        return fail(HEGPU_E_INVALID, "Vector size can not be higher than slot count!");            // :74
    }
    if (mode != 3 && !message && message_size > 0) return fail(HEGPU_E_INVALID, "message is null");
    if (!(scale > 0.0)) return fail(HEGPU_E_INVALID, "Scale out of bounds");                       // :63
    if (mode < 2)
        if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_CKKS_ENCODE, 0, 1))) return r;
    return hip_ret(op_ckks_encode(ctx->c, mode, message, message_size, scalar, scale, (u64*) plain, (u64*) ws,
                                  (hipStream_t) stream), who);
}

int hegpu_ckks_encode(hegpu_context* ctx, const double* message, int message_size, double scale, uint64_t* plain,
                      void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return ckks_encode_any(ctx, 0, message, message_size, 0.0, scale, plain, ws, ws_bytes, stream, "hegpu_ckks_encode");
}
int hegpu_ckks_encode_complex(hegpu_context* ctx, const double* message, int message_size, double scale,
                              uint64_t* plain, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return ckks_encode_any(ctx, 1, message, message_size, 0.0, scale, plain, ws, ws_bytes, stream,
                           "hegpu_ckks_encode_complex");
}
int hegpu_ckks_encode_coeff(hegpu_context* ctx, const double* message, int message_size, double scale, uint64_t* plain,
                            hegpu_stream stream)
{
    return ckks_encode_any(ctx, 2, message, message_size, 0.0, scale, plain, nullptr, 0, stream,
                           "hegpu_ckks_encode_coeff");
}
int hegpu_ckks_encode_scalar(hegpu_context* ctx, double value, double scale, uint64_t* plain, hegpu_stream stream)
{
    return ckks_encode_any(ctx, 3, nullptr, 0, value, scale, plain, nullptr, 0, stream, "hegpu_ckks_encode_scalar");
}

static int ckks_decode_any(hegpu_context* ctx, int mode, const uint64_t* plain, int depth, double scale, double* message,
                           void* ws, size_t ws_bytes, hegpu_stream stream, const char* who)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_depth(ctx->c, depth)) return r;
    if (!(scale > 0.0)) return fail(HEGPU_E_INVALID, "scale must be positive");
    if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_CKKS_DECODE, depth, 1))) return r;
    return hip_ret(op_ckks_decode(ctx->c, mode, (const u64*) plain, depth, scale, message, (u64*) ws,
                                  (hipStream_t) stream), who);
}

int hegpu_ckks_decode(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message, void* ws,
                      size_t ws_bytes, hegpu_stream stream)
{
    return ckks_decode_any(ctx, 0, plain, depth, scale, message, ws, ws_bytes, stream, "hegpu_ckks_decode");
}
int hegpu_ckks_decode_complex(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message,
                              void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return ckks_decode_any(ctx, 1, plain, depth, scale, message, ws, ws_bytes, stream, "hegpu_ckks_decode_complex");
}
int hegpu_ckks_decode_coeff(hegpu_context* ctx, const uint64_t* plain, int depth, double scale, double* message,
                            void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return ckks_decode_any(ctx, 2, plain, depth, scale, message, ws, ws_bytes, stream, "hegpu_ckks_decode_coeff");
}

int hegpu_bfv_noise_rns(hegpu_context* ctx, const uint64_t* ct, const uint64_t* sk, uint64_t* out, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    return hip_ret(op_bfv_noise_rns(ctx->c, (const u64*) ct, (const u64*) sk, (u64*) out, (hipStream_t) stream),
                   "hegpu_bfv_noise_rns");
}

// ---- ciphertext (x) plaintext operations
int hegpu_cipherplain_multiplication(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out,
                                     int limbs, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (limbs <= 0 || limbs > ctx->c.Qp_size) return fail(HEGPU_E_INVALID, "bad limb count");
    return hip_ret(kg_pk_u((const u64*) ct, (const u64*) plain, (u64*) out, ctx->c.plan_qp.mods, ctx->c.n_power, limbs,
                           (hipStream_t) stream),
                   "hegpu_cipherplain_multiplication");
}

int hegpu_ckks_constant_op(hegpu_context* ctx, int op, const uint64_t* ct, double value, uint64_t* out, int limbs,
                           int parts, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (op < 0 || op > 2) return fail(HEGPU_E_INVALID, "unknown constant operation");
    if (int r = check_shape(ctx->c, limbs, parts)) return r;
    if (!constant_in_range(value)) return fail(HEGPU_E_INVALID, "constant out of range");
    return hip_ret(kg_ckks_constant((const u64*) ct, value, (u64*) out, ctx->c.plan_qp.mods, ctx->c.n_power, limbs, parts,
                                    op, (hipStream_t) stream),
                   "hegpu_ckks_constant_op");
}

int hegpu_ckks_gaussian_integer_op(hegpu_context* ctx, int op, const uint64_t* ct, double re, double im, uint64_t* out,
                                   int limbs, int parts, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (op < 0 || op > 1) return fail(HEGPU_E_INVALID, "unknown constant operation");
    if (int r = check_shape(ctx->c, limbs, parts)) return r;
    for (double v : {re, im}) // any finite double, as the reference's NTL conversion (ckks/operator.cu:583-617)
        if (!std::isfinite(v)) return fail(HEGPU_E_INVALID, "constant is not a finite number");
    return guarded([&]() -> int {
        return hip_ret(kg_ckks_gaussian((const u64*) ct, re, im, (u64*) out, ctx->c.tab.psi_half, ctx->c.plan_qp.mods,
                                        ctx->c.n_power, limbs, parts, op, (hipStream_t) stream),
                       "hegpu_ckks_gaussian_integer_op");
    });
}

int hegpu_ckks_mult_i(hegpu_context* ctx, const uint64_t* ct, uint64_t* out, int limbs, int parts, int divide,
                      hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_CKKS)) return r;
    if (int r = check_shape(ctx->c, limbs, parts)) return r;
    return guarded([&]() -> int {
        return hip_ret(kg_ckks_mult_i((const u64*) ct, (u64*) out, ctx->c.tab.psi_half, ctx->c.plan_qp.mods,
                                      ctx->c.n_power, limbs, parts, divide, (hipStream_t) stream),
                       "hegpu_ckks_mult_i");
    });
}

int hegpu_bfv_plain_addsub(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out, int sub,
                           hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    const Context& c = ctx->c;
    return guarded([&]() -> int {
        return hip_ret(kg_bfv_plain_addsub((const u64*) ct, (const u64*) plain, (u64*) out, c.plan_qp.mods,
                                           c.tab.coeff_div_plain_modulus, bfv_plain_scale(c), c.n_power, c.Q_size, sub,
                                           (hipStream_t) stream),
                       "hegpu_bfv_plain_addsub");
    });
}

int hegpu_bfv_plain_to_ntt(hegpu_context* ctx, const uint64_t* plain, uint64_t* out, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    return guarded([&]() -> int {
        return hip_ret(op_bfv_plain_to_ntt(ctx->c, (const u64*) plain, (u64*) out, (hipStream_t) stream),
                       "hegpu_bfv_plain_to_ntt");
    });
}

int hegpu_negacyclic_shift(hegpu_context* ctx, const uint64_t* in, uint64_t* out, int shift, int limbs, int parts,
                           hegpu_stream stream)
{
    NEED_CTX(ctx);
    if ((const void*) in == (const void*) out) return fail(HEGPU_E_INVALID, "negacyclic shift: out must not alias in");
    if (limbs <= 0 || limbs > ctx->c.Qp_size || parts < 1 || parts > 3) return fail(HEGPU_E_INVALID, "bad ciphertext shape");
    if (shift < 0 || shift >= (int) (2 * ctx->c.n)) return fail(HEGPU_E_INVALID, "shift must be in [0, 2N)");
    return hip_ret(kg_negacyclic_shift((const u64*) in, (u64*) out, ctx->c.plan_qp.mods, shift, ctx->c.n_power, limbs,
                                       parts, (hipStream_t) stream),
                   "hegpu_negacyclic_shift");
}

int hegpu_bfv_multiply_plain(hegpu_context* ctx, const uint64_t* ct, const uint64_t* plain, uint64_t* out, void* ws,
                             size_t ws_bytes, hegpu_stream stream)
{
    NEED_CTX(ctx);
    if (int r = check_scheme(ctx->c, SCHEME_BFV)) return r;
    if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, OP_BFV_MULTIPLY_PLAIN, 0, 1))) return r;
    return guarded([&]() -> int {
        return hip_ret(op_bfv_multiply_plain(ctx->c, (const u64*) ct, (const u64*) plain, (u64*) out, (u64*) ws,
                                             (hipStream_t) stream),
                       "hegpu_bfv_multiply_plain");
    });
}

// ---- logic gates (HELogicOperator<CKKS / BFV>): the one-pass combine alone, and the whole gate.  Every argument check
// comes before the context is uploaded: a refusal queues nothing and needs no device.
// what both gate entries look at first: the context, the gate (k: its coefficients), the batch (its sign under the entry's name)
static int gate_head_check(const hegpu_context* ctx, int scheme, int gate, int k[3], int batch, const char* who)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    if (int r = check_scheme(ctx->c, scheme)) return r;
    if (!logic_gate_coefficients(gate, k)) return fail(HEGPU_E_INVALID, std::string(who) + ": unknown gate");
    if (batch < 0) return fail(HEGPU_E_INVALID, std::string(who) + ": batch must not be negative");
    if (int r = check_grid(batch, 2, who)) return r;
    return check_batch(batch);
}

// out against one operand: the operand itself (same address and stride, `limbs` limbs per part) or no common word
static int check_gate_operand(const Span& in, bool may_alias, const Span& out, int batch, const char* who)
{
    if (may_alias && in.p == out.p && in.stride == out.stride && in.item == out.item && (batch == 1 || out.stride >= out.item))
        return 0;
    if (!overlaps_any(out, {in}, batch)) return 0;
    return fail(HEGPU_E_INVALID, std::string(who) + ": out is an operand itself (equal strides and limb counts) or does not overlap it");
}

static int gate_combine_entry(hegpu_context* ctx, int scheme, int gate, const uint64_t* a, uint64_t a_stride, int a_limbs,
                              const uint64_t* b, int b_kind, uint64_t b_stride, int b_limbs, const uint64_t* p,
                              uint64_t p_stride, int p_limbs, double scale_one, uint64_t* out, uint64_t out_stride,
                              int limbs, int batch, hegpu_stream stream, const char* who)
{
    int k[3];
    if (int r = gate_head_check(ctx, scheme, gate, k, batch, who)) return leave(r);
    const Context& c = ctx->c;
    const std::string w = who;
    const bool unary = gate == LOGIC_NOT;
    if (unary ? (b_kind != GATE_B_NONE || b || p) : (b_kind != GATE_B_CIPHER && b_kind != GATE_B_PLAIN))
        return fail(HEGPU_E_INVALID, w + ": NOT takes no second operand and no product, every other gate takes both");
    if (!a || !out || (!unary && (!b || !p))) return fail(HEGPU_E_INVALID, w + ": null argument");
    if (limbs < 1 || limbs > c.Q_size) return fail(HEGPU_E_INVALID, w + ": bad limb count");
    if (a_limbs < limbs || a_limbs > c.Q_size || (!unary && (p_limbs < limbs || p_limbs > c.Q_size)) ||
        (!unary && !(scheme == SCHEME_BFV && b_kind == GATE_B_PLAIN) && (b_limbs < limbs || b_limbs > c.Q_size)))
        return fail(HEGPU_E_INVALID, w + ": an operand has fewer limbs than the result");
    if (scheme == SCHEME_CKKS && !(scale_one > 0 && constant_in_range(scale_one)))
        return fail(HEGPU_E_INVALID, w + ": the scale of the constant one is positive and below 3.4e38");
    const Span res{out, out_stride, ct_words(c, limbs)};
    if (int r = check_gate_operand({a, a_stride, ct_words(c, a_limbs)}, true, res, batch, who)) return r;
    if (!unary) {
        const bool cipher = b_kind == GATE_B_CIPHER;
        const uint64_t b_words = cipher ? ct_words(c, b_limbs) : scheme == SCHEME_BFV ? c.n : ct_words(c, b_limbs, 1);
        if (int r = check_gate_operand({b, b_stride, b_words}, cipher, res, batch, who)) return r;
        if (overlaps_any(res, {{p, p_stride, ct_words(c, p_limbs)}}, batch))
            return fail(HEGPU_E_INVALID, w + ": out must not overlap the product");
    }
    NEED_CTX(ctx);
    const bool bfv = scheme == SCHEME_BFV;
    return hip_ret(rns_gate_combine(bfv, k[0], k[1], k[2], (const u64*) a, a_stride, a_limbs, (const u64*) b, b_kind, b_stride,
                                    b_limbs, (const u64*) p, p_stride, p_limbs, scale_one,
                                    bfv ? c.tab.coeff_div_plain_modulus : nullptr, bfv ? bfv_plain_scale(c) : BfvPlainScale{},
                                    (u64*) out, out_stride, c.plan_qp.mods, c.n_power, limbs, batch, (hipStream_t) stream),
                   who);
}

int hegpu_ckks_gate_combine(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, int a_limbs,
                            const uint64_t* b, int b_kind, uint64_t b_stride, int b_limbs, const uint64_t* p,
                            uint64_t p_stride, int p_limbs, double scale_one, uint64_t* out, uint64_t out_stride, int limbs,
                            int batch, hegpu_stream stream)
{
    return gate_combine_entry(ctx, SCHEME_CKKS, gate, a, a_stride, a_limbs, b, b_kind, b_stride, b_limbs, p, p_stride,
                              p_limbs, scale_one, out, out_stride, limbs, batch, stream, "hegpu_ckks_gate_combine");
}

int hegpu_bfv_gate_combine(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b,
                           int b_kind, uint64_t b_stride, const uint64_t* p, uint64_t p_stride, uint64_t* out,
                           uint64_t out_stride, int batch, hegpu_stream stream)
{
    const int Q = ctx ? ctx->c.Q_size : 0;
    return gate_combine_entry(ctx, SCHEME_BFV, gate, a, a_stride, Q, b, b_kind, b_stride, Q, p, p_stride, Q, 0.0, out,
                              out_stride, Q, batch, stream, "hegpu_bfv_gate_combine");
}

static int logic_gate_entry(hegpu_context* ctx, int scheme, int gate, const uint64_t* a, uint64_t a_stride,
                            const uint64_t* b, int b_kind, uint64_t b_stride, const uint64_t* relin_key, double scale_one,
                            uint64_t* out, uint64_t out_stride, int depth, int batch, void* ws, size_t ws_bytes,
                            hegpu_stream stream, const char* who)
{
    int k[3];
    if (int r = gate_head_check(ctx, scheme, gate, k, batch, who)) return leave(r);
    const Context& c = ctx->c;
    const std::string w = who;
    const bool bfv = scheme == SCHEME_BFV;
    if (int r = check_depth(c, depth)) return r;
    const bool unary = gate == LOGIC_NOT;
    if (unary ? (b_kind != GATE_B_NONE || b) : (b_kind != GATE_B_CIPHER && b_kind != GATE_B_PLAIN))
        return fail(HEGPU_E_INVALID, w + ": NOT takes no second operand, every other gate a ciphertext or a plaintext");
    if (!a || !out || (!unary && !b) || (b_kind == GATE_B_CIPHER && !relin_key))
        return fail(HEGPU_E_INVALID, w + ": null argument");
    const int l = c.Q_size - depth;
    if (!bfv && !unary && l < 2) return fail(HEGPU_E_INVALID, w + ": no modulus left to rescale the product by");
    if (!bfv && !(scale_one > 0 && constant_in_range(scale_one)))
        return fail(HEGPU_E_INVALID, w + ": the scale of the constant one is positive and below 3.4e38");
    const int op = bfv ? OP_BFV_LOGIC_GATE : OP_CKKS_LOGIC_GATE;
    if (!unary)
        if (int r = check_workspace(ws, ws_bytes, hegpu_workspace_bytes(ctx, op, depth, batch))) return r;
    const Span in_a{a, a_stride, ct_words(c, l)}, res{out, out_stride, ct_words(c, bfv || unary ? l : l - 1)};
    if (int r = check_gate_operand(in_a, true, res, batch, who)) return r;
    if (!unary) {
        const bool cipher = b_kind == GATE_B_CIPHER;
        const Span in_b{b, b_stride, cipher ? in_a.item : bfv ? c.n : ct_words(c, l, 1)};
        if (int r = check_gate_operand(in_b, cipher, res, batch, who)) return r;
        if (overlaps_any({(const uint64_t*) ws, 0, ws_bytes / sizeof(uint64_t)}, {res, in_a, in_b}, batch))
            return fail(HEGPU_E_INVALID, w + ": the workspace must overlap neither out nor an operand");
    }
    NEED_CTX(ctx);
    return guarded([&]() -> int {
        if (bfv)
            return hip_ret(op_bfv_logic_gate(c, gate, (const u64*) a, a_stride, (const u64*) b, b_kind, b_stride,
                                             (const u64*) relin_key, (u64*) out, out_stride, batch, (u64*) ws,
                                             (hipStream_t) stream),
                           who);
        return hip_ret(op_ckks_logic_gate(c, gate, (const u64*) a, a_stride, (const u64*) b, b_kind, b_stride,
                                          (const u64*) relin_key, scale_one, (u64*) out, out_stride, depth, batch, (u64*) ws,
                                          (hipStream_t) stream),
                       who);
    });
}

int hegpu_ckks_logic_gate(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b, int b_kind,
                          uint64_t b_stride, const uint64_t* relin_key, double scale_one, uint64_t* out, uint64_t out_stride,
                          int depth, int batch, void* ws, size_t ws_bytes, hegpu_stream stream)
{
    return logic_gate_entry(ctx, SCHEME_CKKS, gate, a, a_stride, b, b_kind, b_stride, relin_key, scale_one, out, out_stride,
                            depth, batch, ws, ws_bytes, stream, "hegpu_ckks_logic_gate");
}

int hegpu_bfv_logic_gate(hegpu_context* ctx, int gate, const uint64_t* a, uint64_t a_stride, const uint64_t* b, int b_kind,
                         uint64_t b_stride, const uint64_t* relin_key, uint64_t* out, uint64_t out_stride, int batch, void* ws,
                         size_t ws_bytes, hegpu_stream stream)
{
    return logic_gate_entry(ctx, SCHEME_BFV, gate, a, a_stride, b, b_kind, b_stride, relin_key, 0.0, out, out_stride, 0,
                            batch, ws, ws_bytes, stream, "hegpu_bfv_logic_gate");
}

// ------------------------------------------------------------------ TFHE
struct hegpu_tfhe_context {
    TfheDev p{};
    std::vector<ulonglong2> htw, hitw, hftw, hfitw;
    ulonglong2* dtw = nullptr;
    ulonglong2* ditw = nullptr;
    ulonglong2* dftw = nullptr;
    ulonglong2* dfitw = nullptr;
    bool uploaded = false;
    int device = -1;           // the device the tables live on (the calling thread's current device at first use)
    bool allow_fp = true;      // option "fp" = 0 keeps the integer blind rotate (read by hegpu_tfhe_prepare_bootkey)
    int ks_pieces = -1;        // option "ks_pieces": workgroups per gate (group) of the key switching, -1 by launch size
    int ks_batched = -1;       // option "ks_batched": key switching with 8 / 12 / 16 gates per workgroup sharing the key rows (tfhe.hip)
    // The layout of a prepared boot key is its header word, read by the blind-rotate kernels themselves in stream order
    // (tfhe.hip: tfhe_blind_rotate) -- nothing about a buffer is remembered on the host.  A buffer whose header is
    // neither layout makes the kernel set this pinned word; the next entry of the context reports it (TFHE_NEED).
    int* bad_key = nullptr;
    // tfhe/context.cu:39-42: ks_stdev = 2^-15 sqrt(2/pi), bk_stdev = 9e-9 sqrt(2/pi)
    double ks_stdev = (1.0 / 32768.0) * 0.7978845608028654, bk_stdev = 9e-9 * 0.7978845608028654;
};

static ulonglong2 fp_pair(u64 w, u64 q)
{
    const double wd = (double) w, wi = wd / (double) q;
    u64 a, b;
    memcpy(&a, &wd, 8);
    memcpy(&b, &wi, 8);
    return make_ulonglong2(a, b);
}

int hegpu_tfhe_context_create(hegpu_tfhe_context** out)
{
    return guarded([&]() -> int {
        if (!out) throw std::invalid_argument("null output");
        hegpu_tfhe_context* h = new hegpu_tfhe_context();
        const u64 q = 1152921504606877697ULL, psi = 1689264667710614ULL; // tfhe/context.cu:23-24
        const int np = 10;
        TfheDev& p = h->p;
        p.mod = make_mod(q);
        std::vector<u64> fwd = host::power_table_bitrev(psi, q, np);
        std::vector<u64> inv = host::power_table_bitrev(host::inv_mod_prime(psi, q), q, np);
        h->htw.resize(1024);
        h->hitw.resize(1024);
        for (int j = 0; j < 1024; j++) {
            h->htw[j] = make_ulonglong2(fwd[j], shoup_companion(fwd[j], q));
            h->hitw[j] = make_ulonglong2(inv[j], shoup_companion(inv[j], q));
        }
        const u64 ninv = host::inv_mod_prime(1024, q), w1n = host::mul_mod(inv[1], ninv, q);
        p.ninv = make_ulonglong2(ninv, shoup_companion(ninv, q));
        p.w1ninv = make_ulonglong2(w1n, shoup_companion(w1n, q));
        p.n = 512; p.N = 1024; p.k = 1; p.bk_l = 2; p.bk_bg_bit = 10;
        p.half_bg = (1 << p.bk_bg_bit) >> 1;
        p.mask_mod = (1 << p.bk_bg_bit) - 1;
        long long sum = 0; // compute_offset, tfhe/context.cu:70-81
        for (int i = 1; i <= p.bk_l; i++) sum += 1LL << (32 - i * p.bk_bg_bit);
        p.offset = (int) (sum * p.half_bg);
        p.ks_base_bit = 2; p.ks_length = 8;
        // FP64 blind rotate: our own 44-bit NTT prime (tfhe.hip)
        {
            const u64 fq = host::find_primes(1024, std::vector<int>{44})[0];
            const u64 fpsi = host::minimal_primitive_root(2048, fq);
            std::vector<u64> ff = host::power_table_bitrev(fpsi, fq, np);
            std::vector<u64> fi = host::power_table_bitrev(host::inv_mod_prime(fpsi, fq), fq, np);
            h->hftw.resize(1024);
            h->hfitw.resize(1024);
            for (int j = 0; j < 1024; j++) {
                h->hftw[j] = fp_pair(ff[j], fq);
                h->hfitw[j] = fp_pair(fi[j], fq);
            }
            const u64 fn = host::inv_mod_prime(1024, fq);
            p.fprime = fq;
            p.fninv = fp_pair(fn, fq);
            p.fw1ninv = fp_pair(host::mul_mod(fi[1], fn, fq), fq);
        }
        *out = h;
        // defaults only, through the setter's own validation (a value it refuses is ignored, not stored)
        for (const char* nm : {"fp", "ks_batched", "ks_pieces"}) {
            std::string env = std::string("HEGPU_TFHE_") + nm;
            for (char& ch : env) ch = (char) toupper((unsigned char) ch);
            long v;
            if (env_long(env.c_str(), &v) && v >= INT_MIN && v <= INT_MAX) (void) hegpu_tfhe_context_set_option(h, nm, (int) v);
        }
        return 0;
    });
}

int hegpu_tfhe_context_set_option(hegpu_tfhe_context* ctx, const char* name, int value)
{
    if (!ctx || !name) return fail(HEGPU_E_INVALID, "null argument");
    if (!strcmp(name, "fp")) {
        if (value < 0 || value > 1) return fail(HEGPU_E_INVALID, "value out of range for option fp");
        ctx->allow_fp = value != 0;
    } else if (!strcmp(name, "ks_pieces")) {
        if (value < -1 || value == 0 || value > 64) return fail(HEGPU_E_INVALID, "value out of range for option ks_pieces");
        ctx->ks_pieces = value;
    } else if (!strcmp(name, "ks_batched")) {
        if (value < -1 || (value > 1 && value != 8 && value != 12 && value != 16))
            return fail(HEGPU_E_INVALID, "value out of range for option ks_batched");
        ctx->ks_batched = value;
    } else {
        return fail(HEGPU_E_INVALID, std::string("unknown option: ") + name);
    }
    return 0;
}

void hegpu_tfhe_context_destroy(hegpu_tfhe_context* ctx)
{
    if (!ctx) return;
    if (ctx->dtw) (void) hipFree(ctx->dtw);
    if (ctx->ditw) (void) hipFree(ctx->ditw);
    if (ctx->dftw) (void) hipFree(ctx->dftw);
    if (ctx->dfitw) (void) hipFree(ctx->dfitw);
    if (ctx->bad_key) (void) hipHostFree(ctx->bad_key);
    delete ctx;
}

long hegpu_tfhe_context_int(const hegpu_tfhe_context* ctx, const char* name)
{
    if (!ctx || !name) return -1;
    const TfheDev& p = ctx->p;
    if (!strcmp(name, "n")) return p.n;
    if (!strcmp(name, "N")) return p.N;
    if (!strcmp(name, "k")) return p.k;
    if (!strcmp(name, "bk_l")) return p.bk_l;
    if (!strcmp(name, "bk_bg_bit")) return p.bk_bg_bit;
    if (!strcmp(name, "ks_base_bit")) return p.ks_base_bit;
    if (!strcmp(name, "ks_length")) return p.ks_length;
    if (!strcmp(name, "offset")) return p.offset;
    if (!strcmp(name, "bootkey_elems")) return (long) p.n * (p.k + 1) * p.bk_l * (p.k + 1) * p.N;
    if (!strcmp(name, "prepared_bootkey_elems"))
        return (long) TFHE_PREP_HEADER + 2L * p.n * (p.k + 1) * p.bk_l * (p.k + 1) * p.N;
    if (!strcmp(name, "kskey_b_elems")) return (long) p.N * p.k * p.ks_length * ((1 << p.ks_base_bit) - 1);
    if (!strcmp(name, "kskey_a_elems")) return (long) p.N * p.k * p.ks_length * ((1 << p.ks_base_bit) - 1) * p.n;
    return -1;
}

uint64_t hegpu_tfhe_prime(const hegpu_tfhe_context* ctx) { return ctx ? ctx->p.mod.q : 0; }

static int tfhe_need(hegpu_tfhe_context* ctx)
{
    if (!ctx) return fail(HEGPU_E_INVALID, "null context");
    if (ctx->uploaded) return 0; // (the bad-key flag is NOT looked at here: hegpu_tfhe_status / the bootstrapping entries own it)
    int cnt = 0;
    if (int r = need_device(&cnt)) return r;
    hipError_t e;
    if ((e = hipMalloc((void**) &ctx->dtw, 1024 * sizeof(ulonglong2))) != hipSuccess) return hip_ret(e, "tfhe upload");
    if ((e = hipMalloc((void**) &ctx->ditw, 1024 * sizeof(ulonglong2))) != hipSuccess) return hip_ret(e, "tfhe upload");
    (void) hipMemcpy(ctx->dtw, ctx->htw.data(), 1024 * sizeof(ulonglong2), hipMemcpyHostToDevice);
    (void) hipMemcpy(ctx->ditw, ctx->hitw.data(), 1024 * sizeof(ulonglong2), hipMemcpyHostToDevice);
    if ((e = hipMalloc((void**) &ctx->dftw, 1024 * sizeof(ulonglong2))) != hipSuccess) return hip_ret(e, "tfhe upload");
    if ((e = hipMalloc((void**) &ctx->dfitw, 1024 * sizeof(ulonglong2))) != hipSuccess) return hip_ret(e, "tfhe upload");
    (void) hipMemcpy(ctx->dftw, ctx->hftw.data(), 1024 * sizeof(ulonglong2), hipMemcpyHostToDevice);
    (void) hipMemcpy(ctx->dfitw, ctx->hfitw.data(), 1024 * sizeof(ulonglong2), hipMemcpyHostToDevice);
    ctx->p.tw = ctx->dtw;
    ctx->p.itw = ctx->ditw;
    ctx->p.ftw = ctx->dftw;
    ctx->p.fitw = ctx->dfitw;
    if ((e = hipHostMalloc((void**) &ctx->bad_key, sizeof(int), hipHostMallocMapped)) != hipSuccess) return hip_ret(e, "tfhe upload");
    *ctx->bad_key = 0;
    ctx->p.bad_key = ctx->bad_key;
    (void) hipGetDevice(&ctx->device);
    ctx->uploaded = true;
    return 0;
}
// The blind rotate reads the prepared key's layout ON THE DEVICE; a buffer that is no prepared key makes the kernel set the
// context's pinned flag and write nothing.  The flag is context-wide (not per stream) and is visible once the kernel that
// set it has finished.  Who consumes it (round 5 let ANY later entry of the context consume it -- an unrelated
// encrypt, or a nested call inside hegpu_tfhe_gate, reported and swallowed it):
//   * hegpu_tfhe_status(ctx, stream): drains `stream`, returns HEGPU_E_INVALID if the flag is set and clears it -- the way
//     to learn about a bad call AT that call (call + status), as the reference checks after each launch (util.cuh:47-55);
//   * the entry of hegpu_tfhe_bootstrapping / _gate / _mux themselves, before they queue anything: a caller that never
//     asks still hears about it at its next bootstrapping, and no gate is left half-queued.
static int tfhe_take_bad_key(hegpu_tfhe_context* ctx)
{
    if (ctx->bad_key && __atomic_exchange_n(ctx->bad_key, 0, __ATOMIC_ACQ_REL))
        return fail(HEGPU_E_INVALID, "a bootstrapping call of this context was handed a buffer that is not a prepared boot "
                                     "key (header word neither 0 nor 1): its outputs were not written");
    return 0;
}
#define TFHE_NEED(ctx)        \
    int r = tfhe_need(ctx);   \
    if (r) return r;          \
    DevGuard dev_guard__((ctx)->device); \
    if (dev_guard__.err != hipSuccess) return hip_ret(dev_guard__.err, "switching to the TFHE context's device")

// tfhe/operator.cu:317-323
static int32_t encode_to_torus32(uint32_t mu, uint32_t m_size)
{
    uint64_t interval = ((1ULL << 63) / m_size) * 2;
    uint64_t phase64 = mu * interval;
    return (int32_t) (phase64 >> 32);
}

int hegpu_tfhe_prepare_bootkey(hegpu_tfhe_context* ctx, const uint64_t* boot_key, uint64_t* prepared,
                               hegpu_stream stream)
{
    if (int rc = check_not_capturing(stream, "hegpu_tfhe_prepare_bootkey", SYNCS)) return rc;
    TFHE_NEED(ctx);
    const TfheDev& p = ctx->p;
    const u64 polys = (u64) p.n * (p.k + 1) * p.bk_l * (p.k + 1);
    int fmt = -1;
    return hip_ret(tfhe_prepare_bootkey(p, (const u64*) boot_key, (u64*) prepared, polys, ctx->allow_fp, &fmt,
                                        (hipStream_t) stream),
                   "hegpu_tfhe_prepare_bootkey");
}

// A query, not part of any launch path: the header word of a prepared key, read after the device has drained (so that it
// is ordered behind whatever stream wrote the buffer).  Every failure is -1 (error codes leaked out as "formats").
// It takes no stream, so check_not_capturing has nothing to ask: during a capture the drain itself fails, the answer is -1
// and the capture is lost (include/hegpu.h says so).
int hegpu_tfhe_prepared_format(hegpu_tfhe_context* ctx, const uint64_t* prepared, int refresh)
{
    (void) refresh; // nothing is remembered any more (kept for the ABI)
    if (tfhe_need(ctx)) return -1;
    DevGuard dev_guard__(ctx->device);
    if (dev_guard__.err != hipSuccess) {
        (void) hip_ret(dev_guard__.err, "switching to the TFHE context's device");
        return -1;
    }
    if (!prepared) {
        (void) fail(HEGPU_E_INVALID, "null prepared boot key");
        return -1;
    }
    uint64_t w = ~0ULL;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&w, prepared, sizeof(w), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void) hip_ret(e, "reading the prepared boot key's header");
        return -1;
    }
    if (w > 1) {
        (void) fail(HEGPU_E_INVALID, "not a prepared boot key (header word is neither 0 nor 1)");
        return -1;
    }
    return (int) w;
}

int hegpu_tfhe_gate_precompute(hegpu_tfhe_context* ctx, int gate, int32_t* out_a, int32_t* out_b,
                               const int32_t* a1, const int32_t* b1, const int32_t* a2, const int32_t* b2,
                               int shape, hegpu_stream stream)
{
    TFHE_NEED(ctx);
    if (shape <= 0) return 0; // an empty batch is a no-op (and the cheapest first call: it places the context's tables)
    int enc, s1, s2, m = 1;
    const int e8 = encode_to_torus32(1, 8), e4 = encode_to_torus32(1, 4);
    switch (gate) { // tfhe/operator.cu:24-198
        case HEGPU_GATE_NAND: enc = e8; s1 = -1; s2 = -1; break;
        case HEGPU_GATE_AND: enc = -e8; s1 = 1; s2 = 1; break;
        case HEGPU_GATE_AND_FIRST_NOT: enc = -e8; s1 = -1; s2 = 1; break;
        case HEGPU_GATE_NOR: enc = -e8; s1 = -1; s2 = -1; break;
        case HEGPU_GATE_OR: enc = e8; s1 = 1; s2 = 1; break;
        case HEGPU_GATE_XNOR: enc = -e4; s1 = -1; s2 = -1; m = 2; break;
        case HEGPU_GATE_XOR: enc = e4; s1 = 1; s2 = 1; m = 2; break;
        case HEGPU_GATE_NOT: enc = 0; s1 = -1; s2 = 1; a2 = nullptr; b2 = nullptr; break;
        default: return fail(HEGPU_E_INVALID, "unknown gate");
    }
    return hip_ret(tfhe_gate_pre(out_a, out_b, a1, b1, a2, b2, enc, s1, s2, m, ctx->p.n, shape, (hipStream_t) stream),
                   "hegpu_tfhe_gate_precompute");
}

int hegpu_tfhe_status(hegpu_tfhe_context* ctx, hegpu_stream stream)
{
    if (int rc = check_not_capturing(stream, "hegpu_tfhe_status", SYNCS)) return rc;
    TFHE_NEED(ctx);
    hipError_t e = hipStreamSynchronize((hipStream_t) stream);
    if (e != hipSuccess) return hip_ret(e, "hegpu_tfhe_status");
    return tfhe_take_bad_key(ctx);
}

// (no look at the flag: the nested calls of hegpu_tfhe_gate / _mux)
static int tfhe_bootstrapping_queue(hegpu_tfhe_context* ctx, const int32_t* in_a, const int32_t* in_b,
                                    const uint64_t* prepared_boot_key, int32_t* out_a, int32_t* out_b, int shape,
                                    hegpu_stream stream)
{
    if (shape <= 0) return 0;
    if (!prepared_boot_key) return fail(HEGPU_E_INVALID, "null prepared boot key");
    return hip_ret(tfhe_blind_rotate(ctx->p, in_a, in_b, (const u64*) prepared_boot_key, out_a, out_b,
                                     encode_to_torus32(1, 8), shape, (hipStream_t) stream),
                   "hegpu_tfhe_bootstrapping");
}

int hegpu_tfhe_bootstrapping(hegpu_tfhe_context* ctx, const int32_t* in_a, const int32_t* in_b,
                             const uint64_t* prepared_boot_key, int32_t* out_a, int32_t* out_b, int shape,
                             hegpu_stream stream)
{
    TFHE_NEED(ctx);
    if ((r = tfhe_take_bad_key(ctx))) return r; // an earlier call's bad key, before anything is queued
    return tfhe_bootstrapping_queue(ctx, in_a, in_b, prepared_boot_key, out_a, out_b, shape, stream);
}

int hegpu_tfhe_key_switching(hegpu_tfhe_context* ctx, const int32_t* in_a, const int32_t* in_b, int32_t* out_a,
                             int32_t* out_b, const int32_t* ks_a, const int32_t* ks_b, int shape,
                             hegpu_stream stream)
{
    TFHE_NEED(ctx);
    if (shape > 0) {
        if (!in_a || !in_b || !out_a || !out_b || !ks_a || !ks_b) return fail(HEGPU_E_INVALID, "hegpu_tfhe_key_switching: null pointer");
        // the split forms zero the outputs before any input is read (tfhe.hip): in and out must be distinct buffers
        // (address ranges compared as integers: the pointers may belong to unrelated allocations)
        const uintptr_t ia = (uintptr_t) in_a, ib = (uintptr_t) in_b, oa = (uintptr_t) out_a, ob = (uintptr_t) out_b;
        const size_t ia_n = (size_t) shape * ctx->p.k * ctx->p.N * 4, ib_n = (size_t) shape * 4, oa_n = (size_t) shape * ctx->p.n * 4;
        auto hit = [](uintptr_t a, size_t an, uintptr_t b, size_t bn) { return a < b + bn && b < a + an; };
        if (hit(ia, ia_n, oa, oa_n) || hit(ia, ia_n, ob, ib_n) || hit(ib, ib_n, oa, oa_n) || hit(ib, ib_n, ob, ib_n))
            return fail(HEGPU_E_INVALID, "hegpu_tfhe_key_switching: the output sample overlaps the input sample");
    }
    return hip_ret(tfhe_key_switching(ctx->p, in_a, in_b, out_a, out_b, ks_a, ks_b, shape, ctx->ks_batched, ctx->ks_pieces, (hipStream_t) stream),
                   "hegpu_tfhe_key_switching");
}

int hegpu_tfhe_gate(hegpu_tfhe_context* ctx, int gate, const int32_t* in1_a, const int32_t* in1_b,
                    const int32_t* in2_a, const int32_t* in2_b, int32_t* out_a, int32_t* out_b,
                    const uint64_t* prepared_boot_key, const int32_t* ks_a, const int32_t* ks_b, int shape, void* ws,
                    size_t ws_bytes, hegpu_stream stream)
{
    TFHE_NEED(ctx);
    const TfheDev& p = ctx->p;
    if (gate == HEGPU_GATE_NOT) // NOT needs no bootstrapping (tfhe/operator.cuh:640-686)
        return hegpu_tfhe_gate_precompute(ctx, gate, out_a, out_b, in1_a, in1_b, nullptr, nullptr, shape, stream);
    if ((r = tfhe_take_bad_key(ctx))) return r; // an earlier call's bad key, before anything of this gate is queued
    const size_t need = ((size_t) p.n + (size_t) p.k * p.N + 2) * shape * sizeof(int32_t);
    if ((r = check_workspace(ws, ws_bytes, need))) return r;
    int32_t* t_a = (int32_t*) ws;
    int32_t* t_b = t_a + (size_t) p.n * shape;
    int32_t* e_a = t_b + shape;
    int32_t* e_b = e_a + (size_t) p.k * p.N * shape;
    if ((r = hegpu_tfhe_gate_precompute(ctx, gate, t_a, t_b, in1_a, in1_b, in2_a, in2_b, shape, stream))) return r;
    if ((r = tfhe_bootstrapping_queue(ctx, t_a, t_b, prepared_boot_key, e_a, e_b, shape, stream))) return r;
    return hegpu_tfhe_key_switching(ctx, e_a, e_b, out_a, out_b, ks_a, ks_b, shape, stream);
}

// ---- TFHE front end (reference tfhe/keygenerator.cu, encryptor.cu, decryptor.cu, operator.cuh:676-800)
static const double TFHE_IH = 1.1547005383792517; // sqrt(16/12), see drbg_torus_gaussian

int hegpu_tfhe_generate_secret_key(hegpu_tfhe_context* ctx, hegpu_rng* rng, int32_t* lwe_key, int32_t* tlwe_key,
                                   hegpu_stream stream)
{
    if (int rc = check_not_capturing(stream, "hegpu_tfhe_generate_secret_key", DRAWS)) return rc;
    TFHE_NEED(ctx);
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    const u64 s0 = rng->r.stream;
    rng->r.stream += 2;
    return hip_ret(tfhe_gen_secret(lwe_key, tlwe_key, ctx->p.n, ctx->p.k * ctx->p.N, rng->r.seed, s0,
                                   (hipStream_t) stream),
                   "hegpu_tfhe_generate_secret_key");
}

int hegpu_tfhe_generate_bootstrapping_key(hegpu_tfhe_context* ctx, hegpu_rng* rng, const int32_t* lwe_key,
                                          const int32_t* tlwe_key, uint64_t* boot_key, int32_t* ks_a, int32_t* ks_b,
                                          void* ws, size_t ws_bytes, hegpu_stream stream)
{
    if (int rc = check_not_capturing(stream, "hegpu_tfhe_generate_bootstrapping_key", DRAWS)) return rc;
    TFHE_NEED(ctx);
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    const TfheDev& p = ctx->p;
    if ((r = check_workspace(ws, ws_bytes, (size_t) p.N * sizeof(u64)))) return r;
    const u64 s0 = rng->r.stream;
    rng->r.stream += 4;
    hipError_t e = tfhe_gen_bootkey(p, (u64*) boot_key, lwe_key, tlwe_key, (u64*) ws, ctx->bk_stdev / TFHE_IH,
                                    rng->r.seed, s0, s0 + 1, (hipStream_t) stream);
    if (e != hipSuccess) return hip_ret(e, "hegpu_tfhe_generate_bootstrapping_key");
    const u64 rows = (u64) p.N * p.k * p.ks_length * ((1 << p.ks_base_bit) - 1);
    return hip_ret(tfhe_lwe_encrypt(ks_a, ks_b, lwe_key, nullptr, 1, tlwe_key, p.ks_base_bit, p.ks_length, p.n, rows,
                                    ctx->ks_stdev / TFHE_IH, rng->r.seed, s0 + 2, s0 + 3, (hipStream_t) stream),
                   "hegpu_tfhe_generate_bootstrapping_key");
}

int hegpu_tfhe_encrypt(hegpu_tfhe_context* ctx, hegpu_rng* rng, const int32_t* lwe_key, const int32_t* messages,
                       int shape, int32_t* out_a, int32_t* out_b, hegpu_stream stream)
{
    if (int rc = check_not_capturing(stream, "hegpu_tfhe_encrypt", DRAWS)) return rc;
    TFHE_NEED(ctx);
    if (!rng) return fail(HEGPU_E_INVALID, "null random generator");
    if (shape <= 0) return fail(HEGPU_E_INVALID, "shape must be positive");
    const u64 s0 = rng->r.stream;
    rng->r.stream += 2;
    return hip_ret(tfhe_lwe_encrypt(out_a, out_b, lwe_key, messages, 0, nullptr, 0, 1, ctx->p.n, (u64) shape,
                                    ctx->ks_stdev / TFHE_IH, rng->r.seed, s0, s0 + 1, (hipStream_t) stream),
                   "hegpu_tfhe_encrypt");
}

int hegpu_tfhe_decrypt_phase(hegpu_tfhe_context* ctx, const int32_t* lwe_key, const int32_t* a, const int32_t* b,
                             int shape, int32_t* phase, hegpu_stream stream)
{
    TFHE_NEED(ctx);
    return hip_ret(tfhe_lwe_phase(a, b, lwe_key, phase, ctx->p.n, shape, (hipStream_t) stream),
                   "hegpu_tfhe_decrypt_phase");
}

int hegpu_tfhe_mux(hegpu_tfhe_context* ctx, const int32_t* in1_a, const int32_t* in1_b, const int32_t* in2_a,
                   const int32_t* in2_b, const int32_t* c_a, const int32_t* c_b, int32_t* out_a, int32_t* out_b,
                   const uint64_t* prepared_boot_key, const int32_t* ks_a, const int32_t* ks_b, int shape, void* ws,
                   size_t ws_bytes, hegpu_stream stream)
{
    TFHE_NEED(ctx);
    const TfheDev& p = ctx->p;
    const size_t kN = (size_t) p.k * p.N;
    const size_t need = ((size_t) p.n + 1 + 2 * (kN + 1)) * shape * sizeof(int32_t);
    if ((r = check_workspace(ws, ws_bytes, need))) return r;
    int32_t* t_a = (int32_t*) ws;
    int32_t* t_b = t_a + (size_t) p.n * shape;
    int32_t* e1_a = t_b + shape;
    int32_t* e1_b = e1_a + kN * shape;
    int32_t* e2_a = e1_b + shape;
    int32_t* e2_b = e2_a + kN * shape;
    if ((r = tfhe_take_bad_key(ctx))) return r;
    // AND(c, in1) and AND(NOT c, in2), bootstrapped; OR of the two extracted samples; key switch
    if ((r = hegpu_tfhe_gate_precompute(ctx, HEGPU_GATE_AND, t_a, t_b, c_a, c_b, in1_a, in1_b, shape, stream))) return r;
    if ((r = tfhe_bootstrapping_queue(ctx, t_a, t_b, prepared_boot_key, e1_a, e1_b, shape, stream))) return r;
    if ((r = hegpu_tfhe_gate_precompute(ctx, HEGPU_GATE_AND_FIRST_NOT, t_a, t_b, c_a, c_b, in2_a, in2_b, shape,
                                        stream)))
        return r;
    if ((r = tfhe_bootstrapping_queue(ctx, t_a, t_b, prepared_boot_key, e2_a, e2_b, shape, stream))) return r;
    hipError_t e = tfhe_gate_pre(e1_a, e1_b, e1_a, e1_b, e2_a, e2_b, encode_to_torus32(1, 8), 1, 1, 1, (int) kN, shape,
                                 (hipStream_t) stream); // OR_pre_computation on the N-dimensional samples
    if (e != hipSuccess) return hip_ret(e, "hegpu_tfhe_mux");
    return hegpu_tfhe_key_switching(ctx, e1_a, e1_b, out_a, out_b, ks_a, ks_b, shape, stream);
}

} // extern "C"
