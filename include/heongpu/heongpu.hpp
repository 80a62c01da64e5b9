// heongpu.hpp -- C++ class layer over the C ABI (include/hegpu.h), mirroring
// the reference's public surface for the hot path so that consumer code reads
// the same:
//   heongpu::HEContext<S> ctx = heongpu::GenHEContext<S>(sec);
//   ctx->set_poly_modulus_degree(n); ctx->set_coeff_modulus_bit_sizes(Q, P); ctx->generate();
//   heongpu::Ciphertext<S> ct(ctx);  heongpu::Relinkey<S> rk(ctx);  heongpu::Galoiskey<S> gk(ctx, shifts);
//   heongpu::HEArithmeticOperator<S> op(ctx);
//   op.multiply(a, b, c); op.relinearize_inplace(c, rk); op.rescale_inplace(c); op.rotate_rows(c, d, gk, 1);
// Reference: src/include/heongpu/heongpu.hpp:9-45, util/schemes.h:15-67,
// util/storagemanager.cuh:23-97, util/devicevector.cuh:17-173,
// host/{bfv,ckks}/{context,ciphertext,evaluationkey,operator}.cuh.
//
// Also here: key generation, encryption / decryption, the encoders and the
// reference's serialization format (save/load of every object, util/serializer.h).
// Objects can alternatively be filled through the `load(std::vector)` members with
// data produced elsewhere (tests: seeded synthetic data in the reference's layouts).
//
// Header-only; link against heongpu_amd/lib/libhegpu.so and the HIP runtime.
#pragma once
#include "../hegpu.h"
#if defined(HEONGPU_WITH_ZLIB)
#include <zlib.h> // serializer::compress / decompress (reference util/serializer.cpp)
#endif
#include <hip/hip_runtime.h>
#if defined(HEONGPU_CUDA_NAMES)
#include "cuda_names.hpp" // lets unmodified consumers of the reference (benchmark/*.cpp) use their cuda* calls
#endif
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <complex>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <istream>
#include <map>
#include <ostream>
#include <sstream>
#include <random>
#include <memory>
#include <mutex>
#include <optional>
#include <unordered_map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include <sys/random.h> // RNGSeed: getrandom

// Names that the reference's public headers bring into the global namespace from GPU-NTT /
// GPU-FFT (thirdparty, unvendored) and that its consumers use unqualified (test/test_bfv_*.cpp:
// Data64, Modulus64, OPERATOR64::mult).
typedef unsigned long long Data64;
typedef std::complex<double> Complex64;
struct Modulus64 { // value, bit length, Barrett constant mu = floor(2^(2 bit + 1) / value)
    Data64 value = 0, bit = 0, mu = 0;
    Modulus64() = default;
    Modulus64(Data64 q) : value(q)
    {
        while ((q >> bit) != 0) bit++;
        mu = q ? (Data64) ((((unsigned __int128) 1) << (2 * bit + 1)) / q) : 0;
    }
};
namespace OPERATOR64 { // host-side modular arithmetic on canonical residues
inline Data64 add(Data64 a, Data64 b, const Modulus64& m) { const Data64 s = a + b; return s >= m.value ? s - m.value : s; }
inline Data64 sub(Data64 a, Data64 b, const Modulus64& m) { const Data64 d = a + m.value - b; return d >= m.value ? d - m.value : d; }
inline Data64 mult(Data64 a, Data64 b, const Modulus64& m) { return (Data64) ((unsigned __int128) a * b % m.value); }
inline Data64 reduce(Data64 a, const Modulus64& m) { return a % m.value; }
inline Data64 exp(Data64 base, Data64 e, const Modulus64& m)
{
    Data64 r = 1 % m.value;
    base %= m.value;
    while (e) { if (e & 1) r = mult(r, base, m); base = mult(base, base, m); e >>= 1; }
    return r;
}
inline Data64 modinv(Data64 a, const Modulus64& m) { return exp(a, m.value - 2, m); } // prime moduli
} // namespace OPERATOR64

namespace heongpu {

using ::Data64;
using ::Modulus64;
using ::Complex64;

enum class Scheme { BFV = 1, CKKS = 2, TFHE = 3 };                           // util/schemes.h:15-20
enum class scheme_type : std::uint8_t { none = 0x0, bfv = 0x1, ckks = 0x2, bgv = 0x3, tfhe = 0x4 }; // util/schemes.h:70-86
enum class sec_level_type : std::uint8_t { none = 0x0, sec128 = 0x1, sec192 = 0x2, sec256 = 0x3 }; // :88-104
enum class storage_type : std::uint8_t { HOST = 0x1, DEVICE = 0x2 };        // util/storagemanager.cuh:23-27
enum class keyswitching_type : std::uint8_t { NONE = 0x0, KEYSWITCHING_METHOD_I = 0x1, KEYSWITCHING_METHOD_II = 0x2 };
enum class encoding : std::uint8_t { SLOT = 0x0, COEFFICIENT = 0x1 };        // util/schemes.h:129-133

// util/storagemanager.cuh:34-97
struct ExecutionOptions {
    hipStream_t stream_ = nullptr;
    storage_type storage_ = storage_type::DEVICE;
    bool keep_initial_condition_ = true;
    ExecutionOptions& set_stream(hipStream_t s) { stream_ = s; return *this; }
    ExecutionOptions& set_storage_type(storage_type s) { storage_ = s; return *this; }
    ExecutionOptions& set_initial_location(bool k) { keep_initial_condition_ = k; return *this; }
};

class HipException : public std::runtime_error { // reference util/util.cuh:25-45 CudaException
  public:
    explicit HipException(const std::string& m) : std::runtime_error(m) {}
};

namespace detail {
inline void check(int rc)
{
    if (rc == 0) return;
    const std::string msg = hegpu_last_error();
    switch (rc) {
        case HEGPU_E_INVALID: throw std::invalid_argument(msg);
        case HEGPU_E_LOGIC: throw std::logic_error(msg);
        case HEGPU_E_RUNTIME: throw std::runtime_error(msg);
        default: throw HipException(msg);
    }
}
inline void hip(hipError_t e)
{
    if (e != hipSuccess) throw HipException(hipGetErrorString(e));
}
// one field of the reference's wire format (util/serializer.h): the object's bytes as they lie in memory
template <typename T> void put(std::ostream& os, const T& v) { os.write((const char*) &v, sizeof(T)); }
template <typename T> void get(std::istream& is, T& v) { is.read((char*) &v, sizeof(T)); }
// every class of this layer starts from a context whose device tables exist
template <typename C> void require_generated(const C& context)
{
    if (!context || !context->context_generated_) throw std::invalid_argument("HEContext is not generated!");
}
} // namespace detail

// ------------------------------------------------------------------ memory pool
// util/memorypool.cuh:38-117.  The reference builds RMM pool_memory_resources; here MemoryPool is a
// caching allocator over hipMalloc: freed blocks go to size-ordered free lists together with the
// stream they were last used on and an event recorded at the free, and are handed out again
// without touching the driver (same stream: stream order is enough; other stream: the new
// stream waits for that event).  hipMallocAsync is deliberately NOT used: on this ROCm the
// default stream-ordered pool returns overlapping buffers (tools/hip_pool_repro.cpp,
// profiles/r1h_hip_pool/repro.txt).  `max` caps what the cache keeps, `initial` is reserved
// up front.  The host-side fields are accepted and ignored: pinned host memory (HostVector, the
// storage manager's parking space) comes straight from hipHostMalloc.
struct MemoryPoolConfig {
    std::optional<float> initial_device_fraction, max_device_fraction;
    std::optional<size_t> initial_device_bytes, max_device_bytes;
    std::optional<float> initial_host_fraction, max_host_fraction;
    std::optional<size_t> initial_host_bytes, max_host_bytes;
    bool use_memory_pool = true;
    static MemoryPoolConfig Defaults() { return MemoryPoolConfig(); }
};

class MemoryPool {
  public:
    // One pool per device: a block cached by the pool of device d is memory of device d.  instance() is the pool of the
    // calling thread's current device (one process driving several GPUs, a thread per device as in the reference's
    // example/basic/9_multi_stream_usage_way1.cpp: every thread works with its own device's pool); a DeviceVector
    // remembers the device it was allocated on and returns its memory there, whichever thread frees it.
    static constexpr int kMaxDevices = 64;
    static MemoryPool& instance(int device)
    {
        static MemoryPool pools[kMaxDevices];
        return pools[(device >= 0 && device < kMaxDevices) ? device : 0];
    }
    static MemoryPool& instance() { return instance(current_device()); }
    static int current_device()
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) { (void) hipGetLastError(); d = 0; }
        return d;
    }
    void initialize() { initialize(MemoryPoolConfig::Defaults()); }
    void initialize(const MemoryPoolConfig& config) // the first call wins, like the reference
    {
        std::lock_guard<std::mutex> lock(mu_);
        if (initialized_) return;
        initialized_ = true;
        warm_copy_paths();
        use_pool_ = config.use_memory_pool;
        if (!use_pool_) return;
        size_t free_b = 0, total_b = 0;
        detail::hip(hipMemGetInfo(&free_b, &total_b));
        auto bytes = [&](const std::optional<float>& frac, const std::optional<size_t>& abs, size_t dflt) {
            if (abs) return *abs;
            if (frac) return (size_t) ((double) free_b * (*frac > 1.0f ? *frac / 100.0 : *frac));
            return dflt;
        };
        max_cached_ = bytes(config.max_device_fraction, config.max_device_bytes, (size_t) -1);
        const size_t initial = std::min(bytes(config.initial_device_fraction, config.initial_device_bytes, 0), max_cached_);
        if (initial) { // one block that later requests are carved from by best fit
            Block b;
            b.bytes = round_up(initial);
            b.arena = true;
            if (hipMalloc((void**) &b.p, b.bytes) == hipSuccess) {
                reserved_ += b.bytes;
                free_.insert({b.bytes, b});
                arena_free_[b.p] = b.bytes;
            } else {
                (void) hipGetLastError();
            }
        }
    }
    void use_memory_pool(bool use) { use_pool_ = use; }
    // The runtime sets up its device <-> pinned-host copy path at the first such copy above 16 KiB: 6 ms on this image
    // (rocprofv3 --hip-runtime-trace), which the reference's harness would book on whichever call copies first (the
    // CKKS decode at N = 8192 read 0.94 ms averaged over ten repeats, 0.10 ms afterwards).  Paid once per process here.
    static void warm_copy_paths()
    {
        static std::once_flag once;
        std::call_once(once, [] {
            void *h = nullptr, *d = nullptr;
            const size_t n = 64u << 10;
            if (hipHostMalloc(&h, n, hipHostMallocDefault) == hipSuccess && hipMalloc(&d, n) == hipSuccess &&
                hipMemsetAsync(d, 0, n, nullptr) == hipSuccess) {
                (void) hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, nullptr);
                (void) hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, nullptr);
                (void) hipStreamSynchronize(nullptr);
            }
            if (d) (void) hipFree(d);
            if (h) (void) hipHostFree(h);
            (void) hipGetLastError();
        });
    }

    void* allocate(size_t size, hipStream_t stream = nullptr)
    {
        if (!initialized_) initialize();
        const size_t g = guard();
        char* p = raw_allocate(size + 2 * g, stream);
        // HEGPU_POOL_POISON=<byte>: fill every new buffer, to expose reads of memory nobody wrote
        static const int poison = [] { const char* e = getenv("HEGPU_POOL_POISON"); return e ? atoi(e) : -1; }();
        if (poison >= 0) detail::hip(hipMemsetAsync(p, poison, size + 2 * g, stream));
        if (g) { // HEGPU_POOL_GUARD=<bytes>: canaries around every buffer, checked when it is freed
            detail::hip(hipMemsetAsync(p, 0xA5, g, stream));
            detail::hip(hipMemsetAsync(p + g + size, 0xA5, g, stream));
            std::lock_guard<std::mutex> lock(mu_);
            guarded_[p + g] = size;
        }
        return p + g;
    }
    void deallocate(void* ptr, size_t size, hipStream_t stream = nullptr)
    {
        if (!ptr) return;
        const size_t g = guard();
        if (g) {
            check_one((char*) ptr, size, "free");
            std::lock_guard<std::mutex> lock(mu_);
            guarded_.erase((char*) ptr);
        }
        raw_deallocate((char*) ptr - g, stream);
    }
    void* host_allocate(size_t size)
    {
        void* p = nullptr;
        detail::hip(hipHostMalloc(&p, size, hipHostMallocDefault));
        return p;
    }
    void host_deallocate(void* p, size_t) { if (p) (void) hipHostFree(p); }
    void print_memory_pool_status() const
    {
        size_t free_b = 0, total_b = 0;
        (void) hipMemGetInfo(&free_b, &total_b);
        const double mb = 1024.0 * 1024.0;
        std::cout << "Device Memory Pool: " << (use_pool_ ? "caching allocator over hipMalloc" : "disabled (hipMalloc)") << std::endl;
        std::cout << "-->   in use: " << in_use_ / mb << " MB, reserved: " << reserved_ / mb << " MB" << std::endl;
        std::cout << "-->   device free: " << free_b / mb << " MB of " << total_b / mb << " MB" << std::endl;
    }
    // give every cached block back to the driver (after the work that last used it has finished)
    void release_cached()
    {
        std::lock_guard<std::mutex> lock(mu_);
        release_cached_locked();
    }
    // debug (HEGPU_POOL_GUARD): verify the canaries of every live buffer
    void check_all(const char* when)
    {
        std::map<char*, size_t> snapshot;
        { std::lock_guard<std::mutex> lock(mu_); snapshot = guarded_; }
        for (const auto& a : snapshot) check_one(a.first, a.second, when);
    }

  private:
    struct Block {
        char* p = nullptr;
        size_t bytes = 0;
        hipStream_t stream = nullptr; // stream of the last use
        hipEvent_t freed = nullptr;   // recorded on `stream` when the block was given back
        bool arena = false;           // piece of the initial reservation (never returned to the driver)
    };
    MemoryPool() = default;
    static size_t round_up(size_t b) // 512 B granules below 1 MiB, 2 MiB granules above
    {
        if (b == 0) b = 1;
        return b <= (1u << 20) ? (b + 511) & ~(size_t) 511 : (b + (2u << 20) - 1) & ~(size_t) ((2u << 20) - 1);
    }
    char* raw_allocate(size_t size, hipStream_t stream)
    {
        if (!use_pool_) {
            char* p = nullptr;
            detail::hip(hipMalloc((void**) &p, size));
            return p;
        }
        const size_t want = round_up(size);
        std::lock_guard<std::mutex> lock(mu_);
        auto it = free_.lower_bound(want);
        // near fit only (at most 1.25x, or anything up to 2 MiB), so that the repeating request
        // sizes of HE pipelines find their own blocks again; pieces of the initial reservation
        // are carved by best fit
        while (it != free_.end() && !(it->first <= want + want / 4 || it->first <= 2 * (1u << 20) || it->second.arena)) ++it;
        Block b;
        if (it != free_.end()) {
            b = it->second;
            free_.erase(it);
            if (b.arena) arena_free_.erase(b.p);
            else cached_ -= b.bytes;
            if (b.arena && b.bytes - want >= (2u << 20)) { // split: the tail stays cached
                Block tail = b;
                tail.p = b.p + want;
                tail.bytes = b.bytes - want;
                tail.freed = nullptr;
                if (b.freed) { // the tail was freed with the same work
                    detail::hip(hipEventCreateWithFlags(&tail.freed, hipEventDisableTiming));
                    detail::hip(hipEventRecord(tail.freed, b.stream));
                }
                free_.insert({tail.bytes, tail});
                arena_free_[tail.p] = tail.bytes;
                b.bytes = want;
            }
            if (b.freed && b.stream != stream) detail::hip(hipStreamWaitEvent(stream, b.freed, 0));
        } else {
            hipError_t e = hipMalloc((void**) &b.p, want);
            if (e != hipSuccess) { // out of memory: drop the cache and try once more
                (void) hipGetLastError();
                release_cached_locked();
                detail::hip(hipMalloc((void**) &b.p, want));
            }
            b.bytes = want;
            reserved_ += want;
        }
        in_use_ += b.bytes;
        live_[b.p] = b;
        return b.p;
    }
    void raw_deallocate(char* p, hipStream_t stream)
    {
        if (!use_pool_) { (void) hipFree(p); return; }
        std::lock_guard<std::mutex> lock(mu_);
        auto it = live_.find(p);
        if (it == live_.end()) { (void) hipFree(p); return; } // allocated before the pool was switched on
        Block b = it->second;
        live_.erase(it);
        in_use_ -= b.bytes;
        b.stream = stream;
        if (!b.freed) (void) hipEventCreateWithFlags(&b.freed, hipEventDisableTiming);
        (void) hipEventRecord(b.freed, stream);
        if (b.arena) { // pieces of the initial reservation coalesce with their free neighbours
            auto next = arena_free_.find(b.p + b.bytes);
            if (next != arena_free_.end()) absorb_locked(b, next->first, next->second, true);
            auto prev = arena_free_.lower_bound(b.p);
            if (prev != arena_free_.begin()) {
                --prev;
                if (prev->first + prev->second == b.p) absorb_locked(b, prev->first, prev->second, false);
            }
            arena_free_[b.p] = b.bytes;
        } else {
            cached_ += b.bytes;
        }
        free_.insert({b.bytes, b});
        // the cap is on what the cache KEEPS (live memory is the caller's business): a working set above
        // it must not turn every free into a device synchronisation
        if (cached_ > max_cached_) release_cached_locked();
    }
    // merge the free arena piece (np, nbytes) into b; the merged block is reusable once both frees are done,
    // so b's stream waits for the neighbour's event and b's event is recorded again
    void absorb_locked(Block& b, char* np, size_t nbytes, bool after)
    {
        auto range = free_.equal_range(nbytes);
        for (auto f = range.first; f != range.second; ++f) {
            if (f->second.p != np) continue;
            Block nb = f->second;
            free_.erase(f);
            arena_free_.erase(np);
            if (nb.freed) {
                (void) hipStreamWaitEvent(b.stream, nb.freed, 0);
                (void) hipEventDestroy(nb.freed);
            }
            (void) hipEventRecord(b.freed, b.stream);
            if (!after) b.p = np;
            b.bytes += nbytes;
            return;
        }
    }
    void release_cached_locked()
    {
        (void) hipDeviceSynchronize();
        for (auto it = free_.begin(); it != free_.end();) {
            Block& b = it->second;
            if (b.arena) { ++it; continue; } // pieces of the initial reservation stay
            if (b.freed) (void) hipEventDestroy(b.freed);
            (void) hipFree(b.p);
            reserved_ -= b.bytes;
            cached_ -= b.bytes;
            it = free_.erase(it);
        }
    }
    void check_one(char* ptr, size_t size, const char* when)
    {
        const size_t g = guard();
        std::vector<unsigned char> h(2 * g);
        (void) hipDeviceSynchronize();
        (void) hipMemcpy(h.data(), ptr - g, g, hipMemcpyDeviceToHost);
        (void) hipMemcpy(h.data() + g, ptr + size, g, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < 2 * g; i++)
            if (h[i] != 0xA5) {
                size_t bad = 0;
                for (size_t k = 0; k < 2 * g; k++) bad += h[k] != 0xA5;
                std::cerr << "MemoryPool guard [" << when << "]: buffer of " << size << " bytes was written "
                          << (i < g ? "before its start" : "past its end") << " (" << bad << " canary bytes differ)" << std::endl;
                break;
            }
    }
    static size_t guard()
    {
        static const size_t g = [] { const char* e = getenv("HEGPU_POOL_GUARD"); return e ? (size_t) atol(e) : (size_t) 0; }();
        return g;
    }
    bool initialized_ = false, use_pool_ = true;
    std::mutex mu_;
    std::multimap<size_t, Block> free_;        // cached blocks by size
    std::unordered_map<char*, Block> live_;    // blocks handed out
    std::map<char*, size_t> guarded_;          // only with HEGPU_POOL_GUARD
    std::map<char*, size_t> arena_free_;       // free pieces of the initial reservation by address (coalescing)
    size_t reserved_ = 0, in_use_ = 0, cached_ = 0, max_cached_ = (size_t) -1; // cached_: free non-arena bytes
};

// util/devicevector.cuh:17-173: stream-ordered device buffer
template <typename T> class DeviceVector {
  public:
    DeviceVector() = default;
    explicit DeviceVector(size_t n, hipStream_t s = nullptr) { resize(n, s); }
    DeviceVector(const std::vector<T>& h, hipStream_t s = nullptr)
    {
        resize(h.size(), s);
        if (!h.empty()) detail::hip(hipMemcpyAsync(p_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    }
    DeviceVector(const DeviceVector& o) { copy_from(o); }
    DeviceVector& operator=(const DeviceVector& o)
    {
        if (this != &o) { release(); copy_from(o); }
        return *this;
    }
    DeviceVector(DeviceVector&& o) noexcept : p_(o.p_), n_(o.n_), s_(o.s_), dev_(o.dev_) { o.p_ = nullptr; o.n_ = 0; }
    // The buffer being replaced was last read by the work that produced `o` (an in-place operator on
    // o's stream), possibly on another stream than the one it was allocated on: free it ordered after both.
    DeviceVector& operator=(DeviceVector&& o) noexcept
    {
        if (this != &o) {
            release(o.dev_ == dev_ ? o.s_ : s_); // a stream of another device cannot order this buffer's release
            p_ = o.p_; n_ = o.n_; s_ = o.s_; dev_ = o.dev_; o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DeviceVector() { release(); }
    void resize(size_t n, hipStream_t s = nullptr)
    {
        release();
        s_ = s;
        n_ = n;
        if (n) {
            dev_ = MemoryPool::current_device(); // the calling thread's device: `s` is one of its streams
            p_ = (T*) MemoryPool::instance(dev_).allocate(n * sizeof(T), s);
        }
    }
    T* data() const { return p_; }
    size_t size() const { return n_; }
    hipStream_t stream() const { return s_; }
    void set_stream(hipStream_t s) { s_ = s; }
    int device() const { return dev_; } // the device the buffer lives on (-1: empty)

  private:
    void release() { release(s_); }
    void release(hipStream_t last_use)
    {
        if (p_) {
            // events and streams of this buffer belong to its device: freed from a thread that works on another one,
            // the release runs with that device current
            const int cur = MemoryPool::current_device();
            if (cur != dev_) (void) hipSetDevice(dev_);
            if (last_use != s_) { // make the freeing stream wait for the allocation stream's work as well
                hipEvent_t e = nullptr;
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) {
                    (void) hipEventRecord(e, s_);
                    (void) hipStreamWaitEvent(last_use, e, 0);
                    (void) hipEventDestroy(e);
                }
            }
            MemoryPool::instance(dev_).deallocate(p_, n_ * sizeof(T), last_use);
            if (cur != dev_) (void) hipSetDevice(cur);
        }
        p_ = nullptr;
        n_ = 0;
    }
    // A copy lives on the COPYING thread's device: copy-constructing a key on device d from the key on device 0 is how
    // a multi-device consumer replicates evaluation keys (a peer copy over xGMI); hegpu_broadcast_key is the C-ABI form.
    void copy_from(const DeviceVector& o)
    {
        const bool same = o.dev_ < 0 || o.dev_ == MemoryPool::current_device();
        resize(o.n_, same ? o.s_ : nullptr);
        if (!n_) return;
        if (same) detail::hip(hipMemcpyAsync(p_, o.p_, n_ * sizeof(T), hipMemcpyDeviceToDevice, s_));
        else {
            // The source may still be in flight on ITS stream (o.s_, on the other device): hipMemcpyPeer orders
            // behind nothing there, so the copy is queued on this buffer's stream behind an event recorded on the
            // source's stream (as hegpu_broadcast_bytes does), then waited for -- the copy constructor's contract is
            // a finished replica.  ADVICE r3.
            hipEvent_t ready = nullptr;
            const int cur = MemoryPool::current_device();
            detail::hip(hipSetDevice(o.dev_));
            hipError_t e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ready, o.s_);
            (void) hipSetDevice(cur);
            detail::hip(e);
            e = hipStreamWaitEvent(s_, ready, 0);
            if (e == hipSuccess) e = hipMemcpyPeerAsync(p_, dev_, o.p_, o.dev_, n_ * sizeof(T), s_);
            if (e == hipSuccess) e = hipStreamSynchronize(s_);
            (void) hipEventDestroy(ready);
            detail::hip(e);
        }
    }
    T* p_ = nullptr;
    size_t n_ = 0;
    hipStream_t s_ = nullptr;
    int dev_ = -1;
};

// util/hostvector.cuh:17-31: host vector in pinned (page-locked) memory, so that the storage manager's
// host <-> device copies are asynchronous DMA transfers (the reference: rmm_pinned_allocator)
template <typename T> struct PinnedAllocator {
    using value_type = T;
    PinnedAllocator() = default;
    template <typename U> PinnedAllocator(const PinnedAllocator<U>&) noexcept {}
    T* allocate(size_t n)
    {
        void* p = nullptr;
        if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); throw std::bad_alloc(); }
        return (T*) p;
    }
    void deallocate(T* p, size_t) noexcept { (void) hipHostFree(p); }
    template <typename U> bool operator==(const PinnedAllocator<U>&) const noexcept { return true; }
    template <typename U> bool operator!=(const PinnedAllocator<U>&) const noexcept { return false; }
};
template <typename T> using HostVector = std::vector<T, PinnedAllocator<T>>;

// ------------------------------------------------------------------ storage manager
// util/storagemanager.cuh:113-275 (input_storage_manager / output_storage_manager) and the
// store_in_host / store_in_device / copy_to_device / remove_from_* methods of every object
// (e.g. ckks/ciphertext.cu:52-169).  An object's residues live either in HBM or in pinned host memory.
// An operator that touches a HOST-stored object stages it on use (an asynchronous copy on the operator's
// stream); when the operator returns, inputs go back to where they were (keep_initial_condition_, with a
// copy-back because the operators take non-const references) or stay on the device, and every object the
// operator wrote is placed where ExecutionOptions::storage_ says.  An object that is both -- the operand of an in-place
// form -- goes back to the host if either rule says so.
namespace detail {
class StoredBuffer;
struct OpScope {
    explicit OpScope(const ExecutionOptions& o) : o_(o), outer_(current() == nullptr), exceptions_(std::uncaught_exceptions())
    {
        if (outer_) current() = this;
    }
    ~OpScope() noexcept(false);
    static OpScope*& current()
    {
        static thread_local OpScope* c = nullptr;
        return c;
    }
    void staged(StoredBuffer* b) { if (std::find(staged_.begin(), staged_.end(), b) == staged_.end()) staged_.push_back(b); }
    void written(StoredBuffer* b) { if (std::find(written_.begin(), written_.end(), b) == written_.end()) written_.push_back(b); }
    // a registered buffer that dies (an operator-local temporary) or moves before the operator returns
    void forget(const StoredBuffer* b)
    {
        staged_.erase(std::remove(staged_.begin(), staged_.end(), b), staged_.end());
        written_.erase(std::remove(written_.begin(), written_.end(), b), written_.end());
    }
    void moved(const StoredBuffer* from, StoredBuffer* to)
    {
        for (auto* v : {&staged_, &written_})
            if (std::find(v->begin(), v->end(), from) != v->end()) {
                v->erase(std::remove(v->begin(), v->end(), from), v->end());
                if (std::find(v->begin(), v->end(), to) == v->end()) v->push_back(to);
            }
    }
    hipStream_t stream() const { return o_.stream_; }

  private:
    ExecutionOptions o_;
    bool outer_;
    int exceptions_; // uncaught exceptions when the operator started: more of them in the destructor = unwinding
    std::vector<StoredBuffer*> staged_, written_;
};

class StoredBuffer {
  public:
    StoredBuffer() = default;
    StoredBuffer(DeviceVector<Data64>&& m) : dev_(std::move(m)) {}
    StoredBuffer(const StoredBuffer& o) : dev_(o.dev_), host_(o.host_), st_(o.st_), staged_(o.staged_) {}
    // Inside an operator (OpScope::current()) an assignment makes this object something the operator wrote: it is
    // placed per ExecutionOptions::storage_ when the operator returns (`out = in` of a zero shift, `out =
    // std::move(cur)` at the end of a key chain).  A buffer the scope knows about unregisters itself when it dies or
    // moves, so the scope never touches an operator-local temporary that is already gone.
    StoredBuffer& operator=(const StoredBuffer& o)
    {
        if (this != &o) {
            dev_ = o.dev_; host_ = o.host_; st_ = o.st_; staged_ = o.staged_;
            if (OpScope* sc = OpScope::current()) sc->written(this);
        }
        return *this;
    }
    StoredBuffer(StoredBuffer&& o) noexcept : dev_(std::move(o.dev_)), host_(std::move(o.host_)), st_(o.st_), staged_(o.staged_)
    {
        if (OpScope* sc = OpScope::current()) sc->moved(&o, this);
    }
    StoredBuffer& operator=(StoredBuffer&& o)
    {
        if (this != &o) {
            dev_ = std::move(o.dev_); host_ = std::move(o.host_); st_ = o.st_; staged_ = o.staged_;
            if (OpScope* sc = OpScope::current()) { sc->forget(&o); sc->written(this); }
        }
        return *this;
    }
    ~StoredBuffer()
    {
        if (OpScope* sc = OpScope::current()) sc->forget(this);
    }
    // fresh residues from an operator: they are on the device, whatever the object held before is gone
    StoredBuffer& operator=(DeviceVector<Data64>&& m)
    {
        dev_ = std::move(m);
        drop_host();
        st_ = storage_type::DEVICE;
        staged_ = false;
        if (OpScope* sc = OpScope::current()) sc->written(this);
        return *this;
    }
    // device address; a HOST-stored object is staged first (on the running operator's stream)
    Data64* data()
    {
        if (st_ == storage_type::HOST && !staged_ && !host_.empty()) {
            OpScope* sc = OpScope::current();
            copy_to_device(sc ? sc->stream() : dev_.stream());
            if (sc) sc->staged(this);
        }
        return dev_.data();
    }
    const Data64* data() const { return const_cast<StoredBuffer*>(this)->data(); }
    size_t size() const { return (st_ == storage_type::HOST && !staged_) ? host_.size() : dev_.size(); }
    hipStream_t stream() const { return dev_.stream(); }
    void set_stream(hipStream_t s) { dev_.set_stream(s); }
    bool is_on_device() const noexcept { return st_ == storage_type::DEVICE; }
    storage_type storage() const noexcept { return st_; }
    void set_storage(storage_type t) { if (size() == 0) st_ = t; } // an empty object only records the wish
    const HostVector<Data64>& host_data() const { return host_; }

    void store_in_device(hipStream_t s = nullptr) // */ciphertext.cu store_in_device
    {
        if (st_ == storage_type::DEVICE) return;
        if (!staged_ && !host_.empty()) upload(s);
        drop_host();
        st_ = storage_type::DEVICE;
        staged_ = false;
    }
    void store_in_host(hipStream_t s = nullptr) // */ciphertext.cu store_in_host
    {
        if (st_ == storage_type::HOST && !staged_) return;
        if (dev_.size()) {
            host_.resize(dev_.size());
            hip(hipMemcpyAsync(host_.data(), dev_.data(), dev_.size() * sizeof(Data64), hipMemcpyDeviceToHost, s));
            hip(hipStreamSynchronize(s)); // the device buffer is released next; the host copy must be complete
            dev_.set_stream(s);
            dev_ = DeviceVector<Data64>();
        }
        st_ = storage_type::HOST;
        staged_ = false;
    }
    void copy_to_device(hipStream_t s = nullptr) // host copy kept: the object still counts as HOST-stored
    {
        if (st_ == storage_type::DEVICE || staged_) return;
        if (!host_.empty()) upload(s);
        staged_ = true;
    }
    void remove_from_device(hipStream_t s = nullptr)
    {
        if (st_ != storage_type::HOST || !staged_) return;
        dev_.set_stream(s);
        dev_ = DeviceVector<Data64>();
        staged_ = false;
    }
    void remove_from_host()
    {
        if (st_ == storage_type::HOST && staged_) { st_ = storage_type::DEVICE; staged_ = false; }
        if (st_ == storage_type::DEVICE) drop_host();
    }
    bool staged() const noexcept { return staged_; }

  private:
    void upload(hipStream_t s)
    {
        DeviceVector<Data64> d(host_.size(), s);
        hip(hipMemcpyAsync(d.data(), host_.data(), host_.size() * sizeof(Data64), hipMemcpyHostToDevice, s));
        dev_ = std::move(d);
    }
    void drop_host() { HostVector<Data64>().swap(host_); }
    DeviceVector<Data64> dev_;
    HostVector<Data64> host_;
    storage_type st_ = storage_type::DEVICE;
    bool staged_ = false;
};

inline OpScope::~OpScope() noexcept(false)
{
    if (!outer_) return;
    current() = nullptr;
    // the operator is leaving through an exception: no copies, no synchronisation (a second throw from here would be
    // std::terminate); staged operands simply stay where they are
    if (std::uncaught_exceptions() > exceptions_) return;
    // what the operator wrote goes where storage_ says; an operand it staged from the host and then overwrote (an in-place
    // form: add_inplace, multiply_inplace) is still an input, and keep_initial_condition_ sends it back to the host
    for (StoredBuffer* b : written_) {
        const bool host_input = std::find(staged_.begin(), staged_.end(), b) != staged_.end();
        if (o_.storage_ == storage_type::HOST || (o_.keep_initial_condition_ && host_input)) b->store_in_host(o_.stream_);
    }
    for (StoredBuffer* b : staged_) {
        if (std::find(written_.begin(), written_.end(), b) != written_.end()) continue;
        if (!b->staged()) continue;
        if (o_.keep_initial_condition_) b->store_in_host(o_.stream_); // back to the host, with what the operator did to it
        else b->remove_from_host();                                    // it lives on the device from now on
    }
}
} // namespace detail

// ------------------------------------------------------------------ context
template <Scheme S> class HEContextImpl { // BFV / CKKS; the TFHE specialisation is at the end of this file

  public:
    explicit HEContextImpl(sec_level_type sec = sec_level_type::sec128) : sec_level_(sec) {}
    ~HEContextImpl() { if (h_) hegpu_context_destroy(h_); }
    HEContextImpl(const HEContextImpl&) = delete;

    void set_poly_modulus_degree(size_t degree) // ckks/context.cu:24-52
    {
        if (coeff_modulus_specified_ || poly_modulus_degree_specified_)
            throw std::logic_error("Poly modulus degree cannot be changed after the coeff_modulus is specified!");
        if (degree == 0 || (degree & (degree - 1))) throw std::logic_error("Poly modulus degree have to be power of two");
        if (degree > 65536 || degree < 4096) throw std::logic_error("Poly modulus degree is not supported");
        n = (int) degree;
        n_power = 0;
        while ((1 << n_power) < n) n_power++;
        poly_modulus_degree_specified_ = true;
    }
    // The chain is fixed here (not in generate()), as in the reference: save() works on a
    // context that has its parameters but no device tables yet (example 13_bfv_serialization).
    void set_coeff_modulus_bit_sizes(const std::vector<int>& q, const std::vector<int>& p) // :54-147
    {
        if (coeff_modulus_specified_ || context_generated_ || !poly_modulus_degree_specified_)
            throw std::logic_error("Coeff_modulus cannot be changed after the context is generated!");
        if (p.empty()) throw std::logic_error("log_P_bases_bit_sizes cannot be empty!");
        hegpu_context* chain = nullptr; // prime search + validation; the scheme tables are built in generate()
        detail::check(hegpu_context_create(HEGPU_CKKS, n, q.data(), (int) q.size(), p.data(), (int) p.size(), 0,
                                           sec_abi(), &chain));
        adopt_chain(chain);
        Q_mod_bit_sizes_ = q;
        P_mod_bit_sizes_ = p;
        Qprime_mod_bit_sizes_ = q;
        Qprime_mod_bit_sizes_.insert(Qprime_mod_bit_sizes_.end(), p.begin(), p.end());
        total_coeff_bit_count = 0;
        for (int b : Qprime_mod_bit_sizes_) total_coeff_bit_count += b;
    }
    // explicit primes (bfv/context.cu:149-265, ckks/context.cu:149-265): the same state machine, validator and security
    // check as the bit-size form; the values themselves must admit a 2N-th root of unity (the reference finds that out
    // in generate(), when its root search fails)
    void set_coeff_modulus_values(const std::vector<Data64>& log_Q_bases, const std::vector<Data64>& log_P_bases)
    {
        if (coeff_modulus_specified_ || context_generated_ || !poly_modulus_degree_specified_)
            throw std::logic_error("Coeff_modulus cannot be changed after the context is generated!");
        if (log_P_bases.empty()) throw std::logic_error("log_P_bases_bit_sizes cannot be empty!");
        std::vector<uint64_t> all(log_Q_bases.begin(), log_Q_bases.end());
        all.insert(all.end(), log_P_bases.begin(), log_P_bases.end());
        detail::check(hegpu_validate_coeff_modulus_values(n, all.data(), (int) log_Q_bases.size(), (int) log_P_bases.size(),
                                                          sec_abi()));
        Q_size = (int) log_Q_bases.size();
        P_size = (int) log_P_bases.size();
        Q_prime_size = Q_size + P_size;
        keyswitching_type_ = P_size == 1 ? keyswitching_type::KEYSWITCHING_METHOD_I : keyswitching_type::KEYSWITCHING_METHOD_II;
        prime_vector_.clear();
        Q_mod_bit_sizes_.clear();
        P_mod_bit_sizes_.clear();
        for (uint64_t v : all) prime_vector_.push_back(Modulus64(v));
        for (int i = 0; i < Q_size; i++) Q_mod_bit_sizes_.push_back((int) prime_vector_[i].bit);
        for (int i = Q_size; i < Q_prime_size; i++) P_mod_bit_sizes_.push_back((int) prime_vector_[i].bit);
        Qprime_mod_bit_sizes_ = Q_mod_bit_sizes_;
        Qprime_mod_bit_sizes_.insert(Qprime_mod_bit_sizes_.end(), P_mod_bit_sizes_.begin(), P_mod_bit_sizes_.end());
        total_coeff_bit_count = 0;
        for (int b : Qprime_mod_bit_sizes_) total_coeff_bit_count += b;
        coeff_modulus_specified_ = true;
    }
    void set_coeff_modulus_default_values(int p_count) // bfv/context.cu:267-374
    {
        if (coeff_modulus_specified_ || context_generated_ || !poly_modulus_degree_specified_)
            throw std::logic_error("Coeff_modulus cannot be changed after the context is generated!");
        if (p_count < 1) throw std::logic_error("P_modulus_size cannot be lower than 1!");
        if (sec_level_ == sec_level_type::none)
            throw std::runtime_error("Invalid security level"); // the default chains exist per level (128 / 192 / 256)
        hegpu_context* chain = nullptr;
        detail::check(hegpu_context_create_default(HEGPU_CKKS, n, p_count, 0, sec_abi(), &chain));
        total_coeff_bit_count = (int) hegpu_context_int(chain, sec_level_ == sec_level_type::sec128   ? "max_logq_128"
                                                               : sec_level_ == sec_level_type::sec192 ? "max_logq_192"
                                                                                                       : "max_logq_256");
        adopt_chain(chain);
        for (int i = 0; i < Q_size; i++) Q_mod_bit_sizes_.push_back((int) prime_vector_[i].bit);
        for (int i = Q_size; i < Q_prime_size; i++) P_mod_bit_sizes_.push_back((int) prime_vector_[i].bit);
    }
    void set_plain_modulus(int t) // bfv/context.cu:376-389
    {
        static_assert(S == Scheme::BFV || S == Scheme::CKKS, "");
        if (context_generated_) throw std::logic_error("Plain modulus cannot be changed after the context is generated!");
        plain_modulus_ = Modulus64((Data64) t);
        plain_modulus_specified_ = true;
    }
    void generate()
    {
        if (context_generated_ || !poly_modulus_degree_specified_ || !coeff_modulus_specified_)
            throw std::logic_error("Context is already generated or parameters are missing!");
        std::vector<uint64_t> primes;
        for (const Modulus64& m : prime_vector_) primes.push_back(m.value);
        detail::check(hegpu_context_create_from_primes((int) S, n, primes.data(), Q_size, P_size, plain_modulus_.value, &h_));
        MemoryPool::instance().initialize();
        detail::check(hegpu_context_upload(h_));
        context_generated_ = true;
    }
    void generate(const MemoryPoolConfig& config) // */context.cu generate(const MemoryPoolConfig&)
    {
        MemoryPool::instance().initialize(config);
        generate();
    }
    void print_parameters() const // */context.cu print_parameters
    {
        if (!context_generated_) { std::cout << "Parameters is not generated yet!" << std::endl; return; }
        std::cout << "==== HEonGPU a GPU Based Homomorphic Encryption Library ====\n" << std::endl;
        std::cout << "Encryption parameters:" << std::endl;
        std::cout << "-->   scheme: " << (S == Scheme::BFV ? "BFV" : "CKKS") << std::endl;
        std::cout << "-->   poly_modulus_degree: " << n << std::endl;
        std::cout << "-->   Q_tilta size: Q( ";
        for (int i = 0; i < Q_size; i++) std::cout << prime_vector_[i].bit << (i + 1 < Q_size ? " + " : "");
        std::cout << " ) + P( ";
        for (int i = Q_size; i < Q_prime_size; i++) std::cout << prime_vector_[i].bit << (i + 1 < Q_prime_size ? " + " : "");
        std::cout << " ) bits" << std::endl;
        if (S == Scheme::BFV) std::cout << "-->   plain_modulus: " << plain_modulus_.value << std::endl;
        std::cout << std::endl;
    }

    // Wire format of */context.cu save/load (bfv :804-930, ckks :576-700): scheme, security
    // level, key-switching type (u8 each), n, n_power, coeff_modulus, total_coeff_bit_count,
    // Q'/Q/P counts (int), then counted arrays: primes (Modulus64), base_q (u64), the three
    // bit-size lists (int); BFV appends the plain modulus (Modulus64).
    void save(std::ostream& os) const
    {
        if (!poly_modulus_degree_specified_ || !coeff_modulus_specified_ || (S == Scheme::BFV && !plain_modulus_specified_))
            throw std::runtime_error("Context has no enough parameters to serialize!");
        detail::put(os, (S == Scheme::BFV) ? scheme_type::bfv : scheme_type::ckks);
        detail::put(os, sec_level_);
        detail::put(os, keyswitching_type_);
        detail::put(os, n);
        detail::put(os, n_power);
        detail::put(os, Q_prime_size); // coeff_modulus
        detail::put(os, total_coeff_bit_count);
        detail::put(os, Q_prime_size);
        detail::put(os, Q_size);
        detail::put(os, P_size);
        write_counted(os, prime_vector_);
        std::vector<Data64> base_q;
        for (const Modulus64& m : prime_vector_) base_q.push_back(m.value);
        write_counted(os, base_q);
        write_counted(os, Qprime_mod_bit_sizes_);
        write_counted(os, Q_mod_bit_sizes_);
        write_counted(os, P_mod_bit_sizes_);
        if (S == Scheme::BFV) detail::put(os, plain_modulus_);
    }
    void load(std::istream& is)
    {
        if (context_generated_ || h_) throw std::runtime_error("Context has been already exist!");
        scheme_type scheme = scheme_type::none;
        detail::get(is, scheme);
        if (scheme != ((S == Scheme::BFV) ? scheme_type::bfv : scheme_type::ckks)) throw std::runtime_error("Invalid scheme binary!");
        int coeff_modulus = 0;
        detail::get(is, sec_level_);
        detail::get(is, keyswitching_type_);
        detail::get(is, n);
        detail::get(is, n_power);
        detail::get(is, coeff_modulus);
        detail::get(is, total_coeff_bit_count);
        detail::get(is, Q_prime_size);
        detail::get(is, Q_size);
        detail::get(is, P_size);
        std::vector<Data64> base_q;
        read_counted(is, prime_vector_);
        read_counted(is, base_q);
        read_counted(is, Qprime_mod_bit_sizes_);
        read_counted(is, Q_mod_bit_sizes_);
        read_counted(is, P_mod_bit_sizes_);
        if (S == Scheme::BFV) detail::get(is, plain_modulus_);
        if (!is || (int) prime_vector_.size() != Q_prime_size || Q_size + P_size != Q_prime_size || n != (1 << n_power))
            throw std::runtime_error("Context binary is not consistent!");
        poly_modulus_degree_specified_ = true;
        coeff_modulus_specified_ = true;
        plain_modulus_specified_ = true;
        this->generate();
    }

    inline int get_poly_modulus_degree() const noexcept { return n; }
    inline int get_ciphertext_modulus_count() const noexcept { return Q_size; }
    inline int get_key_modulus_count() const noexcept { return Q_prime_size; }
    inline std::vector<Data64> get_key_modulus() const
    {
        std::vector<Data64> v;
        for (const Modulus64& m : prime_vector_) v.push_back(m.value);
        return v;
    }
    inline int get_log_poly_modulus_degree() const noexcept { return n_power; }
    inline uint64_t get_plain_modulus() const noexcept { return plain_modulus_.value; }
    hegpu_context* handle() const { return h_; }
    // The device this context's tables live on (generate() uploads them to the calling thread's current device); -1
    // before generate().  Several GPUs in one process: one context per device, each generated and used by a thread
    // that made that device current (hipSetDevice) -- buffers of the class layer are allocated on the calling thread's
    // device (MemoryPool::instance()), the library calls themselves run on the context's device whatever the thread.
    int device() const { return h_ ? hegpu_context_device(h_) : -1; }

    int n = 0, n_power = 0, Q_size = 0, P_size = 0, Q_prime_size = 0;
    int total_coeff_bit_count = 0;
    bool context_generated_ = false;
    keyswitching_type keyswitching_type_ = keyswitching_type::NONE;
    std::vector<Modulus64> prime_vector_;

  private:
    int sec_abi() const
    {
        switch (sec_level_) {
            case sec_level_type::none: return HEGPU_SEC_NONE;
            case sec_level_type::sec128: return HEGPU_SEC_128;
            case sec_level_type::sec192: return HEGPU_SEC_192;
            case sec_level_type::sec256: return HEGPU_SEC_256;
        }
        return -1;
    }
    void adopt_chain(hegpu_context* c) // counts and primes of a host-only context, which is then dropped
    {
        Q_size = (int) hegpu_context_int(c, "Q_size");
        P_size = (int) hegpu_context_int(c, "P_size");
        Q_prime_size = (int) hegpu_context_int(c, "Q_prime_size");
        keyswitching_type_ = P_size == 1 ? keyswitching_type::KEYSWITCHING_METHOD_I
                                         : keyswitching_type::KEYSWITCHING_METHOD_II;
        std::vector<uint64_t> q(Q_prime_size);
        hegpu_context_get(c, "modulus", q.data(), Q_prime_size);
        hegpu_context_destroy(c);
        prime_vector_.clear();
        for (uint64_t v : q) prime_vector_.push_back(Modulus64(v));
        coeff_modulus_specified_ = true;
    }
    template <typename T> static void write_counted(std::ostream& os, const std::vector<T>& v)
    {
        const std::uint32_t count = (std::uint32_t) v.size();
        detail::put(os, count);
        os.write((const char*) v.data(), sizeof(T) * count);
    }
    template <typename T> static void read_counted(std::istream& is, std::vector<T>& v)
    {
        std::uint32_t count = 0;
        detail::get(is, count);
        if (!is || count > (1u << 20)) throw std::runtime_error("Context binary is not consistent!");
        v.resize(count);
        is.read((char*) v.data(), sizeof(T) * count);
    }
    hegpu_context* h_ = nullptr;
    sec_level_type sec_level_;
    Modulus64 plain_modulus_;
    std::vector<int> Qprime_mod_bit_sizes_, Q_mod_bit_sizes_, P_mod_bit_sizes_;
    bool poly_modulus_degree_specified_ = false, coeff_modulus_specified_ = false, plain_modulus_specified_ = false;
};

template <Scheme S> using HEContext = std::shared_ptr<HEContextImpl<S>>;
template <Scheme S> HEContext<S> GenHEContext(sec_level_type sec = sec_level_type::sec128) // util/schemes.h:24-31
{
    return std::make_shared<HEContextImpl<S>>(sec);
}

// ------------------------------------------------------------------ what the stored objects share
namespace detail {
// One buffer of residues in HBM or pinned host memory, and the storage manager's public face for it
// (ckks/ciphertext.cu:52-169 and its copies in every object): Ciphertext, Plaintext, Secretkey, Publickey, Relinkey
// and Switchkey derive from this; Galoiskey keeps a map of StoredBuffer.
class StoredObject {
  public:
    Data64* data() { return buf_.data(); }
    const Data64* data() const { return buf_.data(); }
    void memory_set(DeviceVector<Data64>&& m) { buf_ = std::move(m); }
    void switch_stream(hipStream_t s) { buf_.set_stream(s); }
    hipStream_t stream() const noexcept { return buf_.stream(); }
    bool is_on_device() const noexcept { return buf_.is_on_device(); }
    void store_in_device(hipStream_t s = nullptr) { buf_.store_in_device(s); }
    void store_in_host(hipStream_t s = nullptr) { buf_.store_in_host(s); }
    void copy_to_device(hipStream_t s = nullptr) { buf_.copy_to_device(s); }
    void remove_from_device(hipStream_t s = nullptr) { buf_.remove_from_device(s); }
    void remove_from_host() { buf_.remove_from_host(); }

  protected:
    void download(std::vector<Data64>& out, hipStream_t s) const // get_data, and save() of an object with a stream
    {
        out.resize(buf_.size());
        hip(hipMemcpyAsync(out.data(), buf_.data(), out.size() * sizeof(Data64), hipMemcpyDeviceToHost, s));
        hip(hipStreamSynchronize(s));
    }
    StoredBuffer buf_;
};

// ---- wire format (util/serializer.h): fields through put / get, residues through put_payload / read_payload
inline std::vector<Data64> to_host(const Data64* dev, size_t count)
{
    std::vector<Data64> h(count);
    if (count) hip(hipMemcpy(h.data(), dev, count * sizeof(Data64), hipMemcpyDeviceToHost));
    return h;
}
template <Scheme S> constexpr scheme_type wire_scheme() { return S == Scheme::BFV ? scheme_type::bfv : scheme_type::ckks; }
template <Scheme S> void check_scheme(std::istream& is)
{
    scheme_type sc = scheme_type::none;
    get(is, sc);
    if (sc != wire_scheme<S>()) throw std::runtime_error("Invalid scheme binary!");
}
inline void put_payload(std::ostream& os, const Data64* dev, size_t count)
{
    const std::vector<Data64> h = to_host(dev, count);
    os.write((const char*) h.data(), sizeof(Data64) * count);
}
inline DeviceVector<Data64> read_payload(std::istream& is, size_t count, const char* what)
{
    std::vector<Data64> h(count);
    is.read((char*) h.data(), sizeof(Data64) * count);
    if (!is) throw std::runtime_error(std::string(what) + " binary is truncated!");
    DeviceVector<Data64> d(h);
    hip(hipStreamSynchronize(nullptr));
    return d;
}

// The scratch memory of one C call: ceil(bytes / 8) words on the operator's stream; the call is handed the byte count
// the size query reported.  No bytes, no allocation: data() is null then (a NOT gate).
struct Workspace {
    Workspace(size_t b, hipStream_t s) : bytes(b), words((b + 7) / 8, s) {}
    Workspace(hegpu_context* h, int op, int depth, hipStream_t s) : Workspace(hegpu_workspace_bytes(h, op, depth, 1), s) {}
    Data64* data() const { return words.data(); }
    const size_t bytes;
    DeviceVector<Data64> words;
};

// The shape of a key-switch key (*/evaluationkey.cu:30-36): d digits of 2 x Q' x N residues, with d = Q for one
// special prime (method I) and ceil(Q / m) otherwise, m = 2 (BFV) or P_size (CKKS).  Relinkey, Switchkey and
// Galoiskey derive from it; it also writes and reads the header their wire formats start with.
class KeySwitchShape {
  public:
    KeySwitchShape() = default;
    template <Scheme S> explicit KeySwitchShape(const std::shared_ptr<HEContextImpl<S>>& c)
    {
        require_generated(c);
        const int m = (S == Scheme::BFV) ? 2 : c->P_size;
        ring_size = c->n;
        Q_prime_size_ = c->Q_prime_size;
        Q_size_ = c->Q_size;
        d_ = c->P_size == 1 ? c->Q_size : (c->Q_size + m - 1) / m;
        key_size_ = (Data64) 2 * d_ * Q_prime_size_ * ring_size;
        key_type = c->keyswitching_type_;
    }
    size_t size() const { return (size_t) key_size_; } // elements of one key
    keyswitching_type key_type = keyswitching_type::KEYSWITCHING_METHOD_I;

  protected:
    template <Scheme S> void put_header(std::ostream& os) const // scheme, key type (u8), ring size, Q', Q, d (int)
    {
        put(os, wire_scheme<S>());
        put(os, key_type);
        put(os, ring_size); put(os, Q_prime_size_); put(os, Q_size_); put(os, d_);
    }
    template <Scheme S> void get_header(std::istream& is)
    {
        check_scheme<S>(is);
        get(is, key_type);
        get(is, ring_size); get(is, Q_prime_size_); get(is, Q_size_); get(is, d_);
    }
    int ring_size = 0, Q_prime_size_ = 0, Q_size_ = 0, d_ = 0;
    Data64 key_size_ = 0;
};
} // namespace detail

// ------------------------------------------------------------------ ciphertext
template <Scheme S> class HEArithmeticOperator;
namespace detail {
template <Scheme S> class LogicOperatorBase;
}

template <Scheme S> class Ciphertext : public detail::StoredObject { // host/{ckks,bfv}/ciphertext.cuh
    friend class HEArithmeticOperator<S>;
    friend class detail::LogicOperatorBase<S>;

  public:
    Ciphertext() = default; // filled by load(std::istream&) or by an operator
    explicit Ciphertext(HEContext<S> context, const ExecutionOptions& options = ExecutionOptions())
    {
        detail::require_generated(context);
        ring_size_ = context->n;
        coeff_modulus_count_ = context->Q_size;
        cipher_size_ = 2;
        in_ntt_domain_ = (S == Scheme::CKKS); // CKKS ciphertexts live in the NTT domain (ckks/ciphertext.cu)
        buf_.set_storage(options.storage_);
        buf_.set_stream(options.stream_);
    }
    size_t memory_size() const { return buf_.size(); }
    inline int ring_size() const noexcept { return ring_size_; }
    inline int coeff_modulus_count() const noexcept { return coeff_modulus_count_; }
    inline int size() const noexcept { return cipher_size_; }
    inline int depth() const noexcept { return depth_; }
    inline int level() const noexcept { return coeff_modulus_count_ - (depth_ + 1); } // ckks/ciphertext.cuh:162
    inline double scale() const noexcept { return scale_; }
    inline bool in_ntt_domain() const noexcept { return in_ntt_domain_; }
    inline bool rescale_required() const noexcept { return rescale_required_; }
    inline bool relinearization_required() const noexcept { return relinearization_required_; }
    inline encoding encoding_type() const noexcept { return encoding_; } // CKKS: slots or coefficients
    encoding encoding_ = encoding::SLOT;
    void get_data(std::vector<Data64>& out, hipStream_t s = nullptr) const { download(out, s); }
    // used by the encryptor: take ownership of freshly produced residues
    void adopt(DeviceVector<Data64>&& m, int cipher_size, int depth, double scale)
    {
        buf_ = std::move(m);
        cipher_size_ = cipher_size;
        depth_ = depth;
        scale_ = scale;
        ciphertext_generated_ = true;
        relinearization_required_ = false;
        rescale_required_ = false;
    }
    // Without the encryptor: fill with residues laid out [size][Q - depth][N].
    void load(const std::vector<Data64>& host, int cipher_size, int depth, double scale = 1.0, hipStream_t s = nullptr)
    {
        const size_t want = (size_t) cipher_size * (coeff_modulus_count_ - depth) * ring_size_;
        if (host.size() != want) throw std::invalid_argument("Invalid Ciphertexts size!");
        buf_ = DeviceVector<Data64>(host, s);
        cipher_size_ = cipher_size;
        depth_ = depth;
        scale_ = scale;
        ciphertext_generated_ = true;
        relinearization_required_ = cipher_size == 3;
    }

    // Wire format of the reference, field for field (ckks/ciphertext.cu:171-300,
    // bfv/ciphertext.cu:165-290): scheme (u8), ring size, modulus count, size [, depth] (int),
    // ntt flag (bool), storage (u8) [, scale (double), encoding (u8), rescale flag (bool)],
    // relinearization flag, generated flag (bool), element count (u32), residues (u64).
    void save(std::ostream& os) const
    {
        if (!ciphertext_generated_) throw std::runtime_error("Ciphertext is not generated so can not be serialized!");
        detail::put(os, detail::wire_scheme<S>());
        detail::put(os, ring_size_); detail::put(os, coeff_modulus_count_); detail::put(os, cipher_size_);
        if (S == Scheme::CKKS) detail::put(os, depth_);
        detail::put(os, in_ntt_domain_);
        detail::put(os, storage_type::DEVICE);
        if (S == Scheme::CKKS) { detail::put(os, scale_); detail::put(os, encoding_); detail::put(os, rescale_required_); }
        detail::put(os, relinearization_required_);
        detail::put(os, ciphertext_generated_);
        const std::uint32_t count = (std::uint32_t) ((size_t) cipher_size_ * (coeff_modulus_count_ - depth_) * ring_size_);
        std::vector<Data64> host; // through the object's own stream: the residues may still be in flight there
        download(host, buf_.stream());
        if (host.size() < count) throw std::runtime_error("Ciphertext memory is smaller than its description!");
        detail::put(os, count);
        os.write((const char*) host.data(), sizeof(Data64) * count);
    }
    void load(std::istream& is)
    {
        if (ciphertext_generated_) throw std::runtime_error("Ciphertext has been already exist!");
        detail::check_scheme<S>(is);
        int ring = 0, count_mod = 0;
        detail::get(is, ring); detail::get(is, count_mod);
        if (ring_size_ == 0) { ring_size_ = ring; coeff_modulus_count_ = count_mod; } // default-constructed
        if (ring != ring_size_ || count_mod != coeff_modulus_count_)
            throw std::runtime_error("Ciphertext binary does not match the context!");
        detail::get(is, cipher_size_);
        if (!is || cipher_size_ < 2 || cipher_size_ > 3) throw std::runtime_error("Ciphertext size is not correct!");
        depth_ = 0;
        storage_type st;
        bool generated = false;
        std::uint32_t count = 0;
        if (S == Scheme::CKKS) detail::get(is, depth_);
        detail::get(is, in_ntt_domain_);
        detail::get(is, st);
        if (S == Scheme::CKKS) { detail::get(is, scale_); detail::get(is, encoding_); detail::get(is, rescale_required_); }
        detail::get(is, relinearization_required_);
        detail::get(is, generated);
        detail::get(is, count);
        if (!is || depth_ < 0 || depth_ >= coeff_modulus_count_ ||
            count != (std::uint32_t) ((size_t) cipher_size_ * ring_size_ * (coeff_modulus_count_ - depth_)))
            throw std::runtime_error("Ciphertext size is not correct!");
        std::vector<Data64> host(count);
        is.read((char*) host.data(), sizeof(Data64) * count);
        if (!is) throw std::runtime_error("Ciphertext binary is truncated!");
        buf_ = DeviceVector<Data64>(host, buf_.stream());
        detail::hip(hipStreamSynchronize(buf_.stream()));
        ciphertext_generated_ = true;
    }

  private:
    int ring_size_ = 0, coeff_modulus_count_ = 0, cipher_size_ = 2, depth_ = 0;
    double scale_ = 0;
    bool in_ntt_domain_ = false, rescale_required_ = false, relinearization_required_ = false;
    bool ciphertext_generated_ = false;
};

// ------------------------------------------------------------------ keys
template <Scheme S> class Relinkey : public detail::StoredObject, public detail::KeySwitchShape { // host/*/evaluationkey.cuh
  public:
    Relinkey() = default;
    explicit Relinkey(HEContext<S> context) : detail::KeySwitchShape(context), context_(std::move(context)) {}
    void load(const std::vector<Data64>& host, hipStream_t s = nullptr) // a key produced elsewhere
    {
        if (host.size() != key_size_) throw std::invalid_argument("Invalid relinkey size!");
        buf_ = DeviceVector<Data64>(host, s);
        relin_key_generated_ = true;
    }
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    // */evaluationkey.cu Relinkey::save/load (bfv :91-200): scheme, key type (u8), ring size, Q', Q,
    // d, d_tilda, r_prime (int), storage (u8), generated (bool), element count (u64), the key
    void save(std::ostream& os) const
    {
        if (!relin_key_generated_) throw std::runtime_error("Relinkey is not generated so can not be serialized!");
        put_header<S>(os);
        detail::put(os, d_tilda_); detail::put(os, r_prime_);
        detail::put(os, storage_type::DEVICE);
        detail::put(os, relin_key_generated_);
        detail::put(os, key_size_);
        detail::put_payload(os, buf_.data(), size());
    }
    void load(std::istream& is)
    {
        if (relin_key_generated_) throw std::runtime_error("Relinkey has been already exist!");
        storage_type st;
        get_header<S>(is);
        detail::get(is, d_tilda_); detail::get(is, r_prime_);
        detail::get(is, st);
        detail::get(is, relin_key_generated_);
        detail::get(is, key_size_);
        if (!is || key_size_ > ((Data64) 1 << 36)) throw std::runtime_error("Invalid relinkey size!");
        buf_ = detail::read_payload(is, size(), "Relinkey");
        relin_key_generated_ = true;
    }
    bool relin_key_generated_ = false;

  private:
    HEContext<S> context_;
    int d_tilda_ = 0, r_prime_ = 0;
};

// A key that moves a ciphertext from one secret key to another (host/*/evaluationkey.cuh
// Switchkey; generated by HEKeyGenerator::generate_switch_key, used by keyswitch())
template <Scheme S> class Switchkey : public detail::StoredObject, public detail::KeySwitchShape {
  public:
    Switchkey() = default;
    explicit Switchkey(HEContext<S> context) : detail::KeySwitchShape(context), context_(std::move(context)) {}
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    void save(std::ostream& os) const // */evaluationkey.cu Switchkey::save (bfv :835-882)
    {
        if (!switch_key_generated_) throw std::runtime_error("Switchkey is not generated so can not be serialized!");
        put_header<S>(os);
        detail::put(os, storage_type::DEVICE);
        detail::put(os, switch_key_generated_);
        detail::put(os, key_size_);
        detail::put_payload(os, buf_.data(), size());
    }
    void load(std::istream& is)
    {
        if (switch_key_generated_) throw std::runtime_error("Switchkey has been already exist!");
        storage_type st;
        get_header<S>(is);
        detail::get(is, st);
        detail::get(is, switch_key_generated_);
        detail::get(is, key_size_);
        if (!is || key_size_ > ((Data64) 1 << 36)) throw std::runtime_error("Invalid switchkey size!");
        buf_ = detail::read_payload(is, size(), "Switchkey");
        switch_key_generated_ = true;
    }
    bool switch_key_generated_ = false;

  private:
    HEContext<S> context_;
};

template <Scheme S> class Galoiskey : public detail::KeySwitchShape { // host/*/evaluationkey.cuh; keygeneration.cu:684-728
  public:
    Galoiskey() = default;
    // power-of-two shifts in both directions (evaluationkey.cu:291-345, MAX_SHIFT = 8)
    explicit Galoiskey(HEContext<S> context) : Galoiskey(context, default_shifts()) {}
    static std::vector<int> default_shifts()
    {
        std::vector<int> v;
        for (int i = 0; i < 8; i++) { v.push_back(1 << i); v.push_back(-(1 << i)); }
        return v;
    }
    Galoiskey(HEContext<S> context, const std::vector<int>& shifts) : Galoiskey(std::move(context), false)
    {
        for (int sh : shifts) galois_elt[sh] = hegpu_steps_to_galois_elt(sh, context_->n, group_order_);
    }
    // keys for explicit Galois elements (evaluationkey.cu:347-375)
    Galoiskey(HEContext<S> context, const std::vector<uint32_t>& galois_elts) : Galoiskey(std::move(context), true)
    {
        custom_galois_elt = galois_elts;
    }
    void load(int galois_element, const std::vector<Data64>& host, hipStream_t s = nullptr)
    {
        if (host.size() != key_size_) throw std::invalid_argument("Invalid galoiskey size!");
        device_location_[galois_element] = DeviceVector<Data64>(host, s);
    }
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    // storage manager, every element
    bool is_on_device() const noexcept { for (const auto& k : device_location_) if (!k.second.is_on_device()) return false; return true; }
    void store_in_device(hipStream_t s = nullptr) { each_key(&detail::StoredBuffer::store_in_device, s); }
    void store_in_host(hipStream_t s = nullptr) { each_key(&detail::StoredBuffer::store_in_host, s); }
    void copy_to_device(hipStream_t s = nullptr) { each_key(&detail::StoredBuffer::copy_to_device, s); }
    void remove_from_device(hipStream_t s = nullptr) { each_key(&detail::StoredBuffer::remove_from_device, s); }
    void remove_from_host() { each_key(&detail::StoredBuffer::remove_from_host); }
    // */evaluationkey.cu Galoiskey::save/load (bfv :540-760): header as Relinkey up to d, then
    // customized (bool), group order (int), storage (u8), generated (bool); the element table
    // (u32 list when customized, else (shift, element) int pairs); galois_elt_zero (int), key
    // size (u64), key count (u32), then (element (int), key) per key, and last the key of
    // galois_elt_zero.  The reference keeps that one apart (zero_device_location_); here it sits
    // in the map under its element and is written in the reference's position.
    void save(std::ostream& os) const
    {
        if (!galois_key_generated_) throw std::runtime_error("Galoiskey is not generated so can not be serialized!");
        put_header<S>(os);
        detail::put(os, customized);
        detail::put(os, group_order_);
        detail::put(os, storage_type::DEVICE);
        detail::put(os, galois_key_generated_);
        if (customized) {
            detail::put(os, (std::uint32_t) custom_galois_elt.size());
            os.write((const char*) custom_galois_elt.data(), sizeof(std::uint32_t) * custom_galois_elt.size());
        } else {
            detail::put(os, (std::uint32_t) galois_elt.size());
            for (const auto& g : galois_elt) { detail::put(os, g.first); detail::put(os, g.second); }
        }
        detail::put(os, galois_elt_zero);
        detail::put(os, key_size_);
        // a shift whose element equals galois_elt_zero cannot occur (the latter is 2N-1 / 2N-1)
        std::uint32_t key_count = 0;
        for (const auto& k : device_location_) if (k.first != galois_elt_zero) key_count++;
        detail::put(os, key_count);
        for (const auto& k : device_location_) {
            if (k.first == galois_elt_zero) continue;
            detail::put(os, k.first);
            detail::put_payload(os, k.second.data(), size());
        }
        const auto zero = device_location_.find(galois_elt_zero);
        if (zero == device_location_.end()) throw std::runtime_error("Galoiskey has no column-rotation key!");
        detail::put_payload(os, zero->second.data(), size());
    }
    void load(std::istream& is)
    {
        if (galois_key_generated_) throw std::runtime_error("Galoiskey has been already exist!");
        storage_type st;
        get_header<S>(is);
        detail::get(is, customized);
        detail::get(is, group_order_);
        detail::get(is, st);
        detail::get(is, galois_key_generated_);
        std::uint32_t count = 0;
        detail::get(is, count);
        if (!is || count > (1u << 20)) throw std::runtime_error("Invalid galoiskey binary!");
        galois_elt.clear();
        custom_galois_elt.clear();
        if (customized) {
            custom_galois_elt.resize(count);
            is.read((char*) custom_galois_elt.data(), sizeof(std::uint32_t) * count);
        } else {
            for (std::uint32_t i = 0; i < count; i++) {
                int shift = 0, elt = 0;
                detail::get(is, shift); detail::get(is, elt);
                galois_elt[shift] = elt;
            }
        }
        detail::get(is, galois_elt_zero);
        detail::get(is, key_size_);
        std::uint32_t key_count = 0;
        detail::get(is, key_count);
        if (!is || key_size_ > ((Data64) 1 << 36) || key_count > (1u << 20)) throw std::runtime_error("Invalid galoiskey size!");
        device_location_.clear();
        for (std::uint32_t i = 0; i < key_count; i++) {
            int elt = 0;
            detail::get(is, elt);
            device_location_[elt] = detail::read_payload(is, size(), "Galoiskey");
        }
        device_location_[galois_elt_zero] = detail::read_payload(is, size(), "Galoiskey");
        galois_key_generated_ = true;
    }
    bool galois_key_generated_ = false;
    bool customized = false;
    int galois_elt_zero = 0;
    std::map<int, int> galois_elt;                           // shift -> Galois element
    std::vector<std::uint32_t> custom_galois_elt;            // customized == true
    std::map<int, detail::StoredBuffer> device_location_;    // Galois element -> key (HBM or pinned host memory)
    int group_order_ = 5;

  private:
    Galoiskey(HEContext<S> context, bool custom)
        : detail::KeySwitchShape(context), customized(custom), context_(std::move(context))
    {
        group_order_ = (S == Scheme::BFV) ? 3 : 5; // bfv/evaluationkey.cu:308, ckks/evaluationkey.cu:408
        galois_elt_zero = hegpu_steps_to_galois_elt(0, context_->n, group_order_); // column rotation / conjugation
    }
    template <typename... A> void each_key(void (detail::StoredBuffer::*f)(A...), A... a)
    {
        for (auto& k : device_location_) (k.second.*f)(a...);
    }
    HEContext<S> context_;
};

namespace detail {
// the device address of the key of a Galois element (a HOST-stored key is staged), null when the Galoiskey has none;
// by shift: through the element the shift maps to, which is handed back as well
template <Scheme S> const uint64_t* key_for(Galoiskey<S>& gk, int element)
{
    const auto it = gk.device_location_.find(element);
    return it == gk.device_location_.end() ? nullptr : (const uint64_t*) it->second.data();
}
template <Scheme S> const uint64_t* key_for_shift(Galoiskey<S>& gk, int shift, int ring_size, int& element)
{
    element = hegpu_steps_to_galois_elt(shift, ring_size, gk.group_order_);
    return key_for(gk, element);
}
} // namespace detail

// ------------------------------------------------------------------ secret / public key, plaintext
template <Scheme S> class Secretkey : public detail::StoredObject { // host/*/secretkey.cuh; [Q'][N], NTT domain
  public:
    Secretkey() = default;
    explicit Secretkey(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
        ring_size_ = context_->n;
        coeff_modulus_count_ = context_->Q_prime_size;
        n_power_ = context_->n_power;
        hamming_weight_ = context_->n >> 1; // secretkey.cu:23
    }
    Secretkey(HEContext<S> context, int hamming_weight) : Secretkey(std::move(context))
    {
        if (hamming_weight <= 0 || hamming_weight > ring_size_)
            throw std::invalid_argument("hamming weight has to be in range 0 to ring size."); // secretkey.cu:43
        hamming_weight_ = hamming_weight;
    }
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    inline int ring_size() const noexcept { return ring_size_; }
    inline int coeff_modulus_count() const noexcept { return coeff_modulus_count_; }
    // */secretkey.cu:235-345: scheme (u8), ring size, modulus count, n_power, hamming weight (int),
    // ntt flag, generated flag (bool), storage (u8), element count (u32), residues
    void save(std::ostream& os) const
    {
        if (!secret_key_generated_) throw std::runtime_error("Secretkey is not generated so can not be serialized!");
        const bool ntt = true;
        detail::put(os, detail::wire_scheme<S>());
        detail::put(os, ring_size_); detail::put(os, coeff_modulus_count_); detail::put(os, n_power_);
        detail::put(os, hamming_weight_);
        detail::put(os, ntt);
        detail::put(os, secret_key_generated_);
        detail::put(os, storage_type::DEVICE);
        const std::uint32_t count = (std::uint32_t) ((size_t) coeff_modulus_count_ * ring_size_);
        detail::put(os, count);
        detail::put_payload(os, buf_.data(), count);
    }
    void load(std::istream& is)
    {
        if (secret_key_generated_) throw std::runtime_error("Secretkey has been already exist!");
        detail::check_scheme<S>(is);
        bool ntt = false;
        storage_type st;
        detail::get(is, ring_size_); detail::get(is, coeff_modulus_count_); detail::get(is, n_power_);
        detail::get(is, hamming_weight_);
        detail::get(is, ntt);
        detail::get(is, secret_key_generated_);
        detail::get(is, st);
        std::uint32_t count = 0;
        detail::get(is, count);
        if (!is || ring_size_ <= 0 || coeff_modulus_count_ <= 0 || count != (std::uint32_t) ((size_t) ring_size_ * coeff_modulus_count_))
            throw std::runtime_error("Invalid secretkey size!");
        buf_ = detail::read_payload(is, count, "Secretkey");
        secret_key_generated_ = true;
    }
    int hamming_weight_ = 0;
    bool secret_key_generated_ = false;

  private:
    HEContext<S> context_;
    int ring_size_ = 0, coeff_modulus_count_ = 0, n_power_ = 0;
};

template <Scheme S> class Publickey : public detail::StoredObject { // host/*/publickey.cuh; [2][Q'][N], NTT domain
  public:
    Publickey() = default;
    explicit Publickey(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
        ring_size_ = context_->n;
        coeff_modulus_count_ = context_->Q_prime_size;
    }
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    inline int ring_size() const noexcept { return ring_size_; }
    inline int coeff_modulus_count() const noexcept { return coeff_modulus_count_; }
    // */publickey.cu:92-200: scheme (u8), ring size, modulus count (int), ntt flag, generated flag
    // (bool), storage (u8), element count (u32), residues
    void save(std::ostream& os) const
    {
        if (!public_key_generated_) throw std::runtime_error("Publickey is not generated so can not be serialized!");
        const bool ntt = true;
        detail::put(os, detail::wire_scheme<S>());
        detail::put(os, ring_size_); detail::put(os, coeff_modulus_count_);
        detail::put(os, ntt);
        detail::put(os, public_key_generated_);
        detail::put(os, storage_type::DEVICE);
        const std::uint32_t count = (std::uint32_t) ((size_t) 2 * coeff_modulus_count_ * ring_size_);
        detail::put(os, count);
        detail::put_payload(os, buf_.data(), count);
    }
    void load(std::istream& is)
    {
        if (public_key_generated_) throw std::runtime_error("Publickey has been already exist!");
        detail::check_scheme<S>(is);
        bool ntt = false;
        storage_type st;
        detail::get(is, ring_size_); detail::get(is, coeff_modulus_count_);
        detail::get(is, ntt);
        detail::get(is, public_key_generated_);
        detail::get(is, st);
        std::uint32_t count = 0;
        detail::get(is, count);
        if (!is || ring_size_ <= 0 || coeff_modulus_count_ <= 0 || count != (std::uint32_t) ((size_t) 2 * ring_size_ * coeff_modulus_count_))
            throw std::runtime_error("Invalid publickey size!");
        buf_ = detail::read_payload(is, count, "Publickey");
        public_key_generated_ = true;
    }
    bool public_key_generated_ = false;

  private:
    HEContext<S> context_;
    int ring_size_ = 0, coeff_modulus_count_ = 0;
};

// host/*/plaintext.cuh -- CKKS: [Q - depth][N] NTT domain (+ depth, scale); BFV: [N] mod t
template <Scheme S> class Plaintext : public detail::StoredObject {
  public:
    Plaintext() = default;
    explicit Plaintext(HEContext<S> context, const ExecutionOptions& options = ExecutionOptions())
        : context_(std::move(context))
    {
        detail::require_generated(context_);
        buf_.set_stream(options.stream_);
    }
    size_t size() const { return buf_.size(); }
    void set_context(HEContext<S> context) { context_ = std::move(context); }
    // residues produced elsewhere: [Q - depth][N] of the scaled message, NTT domain (CKKS) / [N] mod t (BFV)
    void load(const std::vector<Data64>& host, int depth, double scale, hipStream_t s = nullptr)
    {
        const size_t want = (S == Scheme::CKKS) ? (size_t) (context_->Q_size - depth) * context_->n : (size_t) context_->n;
        if (host.size() != want) throw std::invalid_argument("Invalid plaintext size!");
        buf_ = DeviceVector<Data64>(host, s);
        depth_ = depth;
        scale_ = scale;
        plaintext_generated_ = true;
    }
    void get_data(std::vector<Data64>& out, hipStream_t s = nullptr) const { download(out, s); }
    // */plaintext.cu (bfv :88-180, ckks :91-200): scheme (u8), size (int) [, depth (int), scale
    // (double)], ntt flag (bool) [, encoding (u8)], generated flag (bool), storage (u8), size again
    // (int), coefficients
    void save(std::ostream& os) const
    {
        if (!plaintext_generated_) throw std::runtime_error("Plaintext is not generated so can not be serialized!");
        const int plain_size = (int) buf_.size();
        const bool ntt = (S == Scheme::CKKS) || in_ntt_domain_;
        detail::put(os, detail::wire_scheme<S>());
        detail::put(os, plain_size);
        if (S == Scheme::CKKS) { detail::put(os, depth_); detail::put(os, scale_); }
        detail::put(os, ntt);
        if (S == Scheme::CKKS) detail::put(os, encoding_);
        detail::put(os, plaintext_generated_);
        detail::put(os, storage_type::DEVICE);
        detail::put(os, plain_size);
        detail::put_payload(os, buf_.data(), (size_t) plain_size);
    }
    void load(std::istream& is)
    {
        if (plaintext_generated_) throw std::runtime_error("Plaintext has been already exist!");
        detail::check_scheme<S>(is);
        int plain_size = 0, again = 0;
        bool ntt = false;
        storage_type st;
        detail::get(is, plain_size);
        if (S == Scheme::CKKS) { detail::get(is, depth_); detail::get(is, scale_); }
        detail::get(is, ntt);
        in_ntt_domain_ = (S == Scheme::BFV) && ntt;
        if (S == Scheme::CKKS) detail::get(is, encoding_);
        detail::get(is, plaintext_generated_);
        detail::get(is, st);
        detail::get(is, again);
        if (!is || plain_size <= 0 || again != plain_size) throw std::runtime_error("Invalid plaintext size!");
        buf_ = detail::read_payload(is, (size_t) plain_size, "Plaintext");
        plaintext_generated_ = true;
    }
    inline int depth() const noexcept { return depth_; }
    inline double scale() const noexcept { return scale_; }
    inline encoding encoding_type() const noexcept { return encoding_; }
    int depth_ = 0;
    double scale_ = 0;
    encoding encoding_ = encoding::SLOT;
    bool in_ntt_domain_ = false; // BFV: after transform_to_ntt ([Q][N] residues instead of [N] mod t)
    bool plaintext_generated_ = false;

  private:
    HEContext<S> context_;
};

// ------------------------------------------------------------------ key generator / encryptor / decryptor
// Key-switching methods I and II (one or several special primes).  Random values come from the backend's DRBG
// (csrc/drbg.hpp: ChaCha20 in counter mode); like the reference's AES generator it is seeded from the
// operating system (256 bits) unless a test seed is given.
template <Scheme S> class HEKeyGenerator { // host/*/keygenerator.cuh
  public:
    // 256 bits of operating-system entropy (getrandom) key the ChaCha20 DRBG
    explicit HEKeyGenerator(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
        detail::check(hegpu_rng_create_from_entropy(&rng_));
    }
    // REPRODUCIBLE TESTS ONLY: a 64-bit seed can be searched exhaustively
    HEKeyGenerator(HEContext<S> context, std::uint64_t seed) : context_(std::move(context))
    {
        detail::require_generated(context_);
        detail::check(hegpu_rng_create(seed, &rng_));
    }
    ~HEKeyGenerator() { hegpu_rng_destroy(rng_); }
    HEKeyGenerator(const HEKeyGenerator&) = delete;
    HEKeyGenerator& operator=(const HEKeyGenerator&) = delete;

    void generate_secret_key(Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (sk.secret_key_generated_) throw std::logic_error("Secretkey is already generated!");
        DeviceVector<Data64> out((size_t) context_->Q_prime_size * context_->n, o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_KEYGEN_SECRET, 0, o.stream_);
        detail::check(hegpu_generate_secret_key(context_->handle(), rng_, sk.hamming_weight_, (uint64_t*) out.data(),
                                                ws.data(), ws.bytes, o.stream_));
        sk.memory_set(std::move(out));
        sk.secret_key_generated_ = true;
    }
    // ckks/keygenerator.cu:85-160: the sampler hegpu_generate_secret_key restates is this one (exactly hamming_weight_
    // non-zero coefficients), so the two names are one function here
    void generate_secret_key_v2(Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions()) { generate_secret_key(sk, o); }
    void generate_public_key(Publickey<S>& pk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (pk.public_key_generated_) throw std::logic_error("Publickey is already generated!");
        DeviceVector<Data64> out((size_t) 2 * context_->Q_prime_size * context_->n, o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_KEYGEN_PUBLIC, 0, o.stream_);
        detail::check(hegpu_generate_public_key(context_->handle(), rng_, (const uint64_t*) sk.data(),
                                                (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
        pk.memory_set(std::move(out));
        pk.public_key_generated_ = true;
    }
    void generate_relin_key(Relinkey<S>& rk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (rk.relin_key_generated_) throw std::logic_error("Relinkey is already generated!");
        DeviceVector<Data64> out(rk.size(), o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_KEYGEN_SWITCH, 0, o.stream_);
        detail::check(hegpu_generate_relin_key(context_->handle(), rng_, (const uint64_t*) sk.data(),
                                               (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
        rk.memory_set(std::move(out));
        rk.relin_key_generated_ = true;
    }
    // key under new_sk that carries old_sk (ckks/keygenerator.cu:996-1095)
    void generate_switch_key(Switchkey<S>& swk, Secretkey<S>& new_sk, Secretkey<S>& old_sk,
                             const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!old_sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (!new_sk.secret_key_generated_) throw std::logic_error("Ner Secretkey is not generated!");
        if (swk.switch_key_generated_) throw std::logic_error("Switchkey is already generated!");
        DeviceVector<Data64> out(swk.size(), o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_KEYGEN_SWITCH, 0, o.stream_);
        detail::check(hegpu_generate_switch_key(context_->handle(), rng_, (const uint64_t*) new_sk.data(),
                                                (const uint64_t*) old_sk.data(), (uint64_t*) out.data(), ws.data(),
                                                ws.bytes, o.stream_));
        swk.memory_set(std::move(out));
        swk.switch_key_generated_ = true;
    }
    void generate_galois_key(Galoiskey<S>& gk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (gk.galois_key_generated_) throw std::logic_error("Galoiskey is already generated!");
        detail::Workspace ws(context_->handle(), HEGPU_OP_KEYGEN_SWITCH, 0, o.stream_);
        std::vector<int> elements; // in the key's own order, the "Columns Rotate" key last (keygenerator.cu:508-560)
        if (gk.customized) for (std::uint32_t e : gk.custom_galois_elt) elements.push_back((int) e);
        else for (auto& g : gk.galois_elt) elements.push_back(g.second);
        elements.push_back(gk.galois_elt_zero);
        for (int elt : elements) {
            if (gk.device_location_.count(elt)) continue;
            DeviceVector<Data64> out(gk.size(), o.stream_);
            detail::check(hegpu_generate_galois_key(context_->handle(), rng_, (const uint64_t*) sk.data(), elt,
                                                    (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
            gk.device_location_[elt] = std::move(out);
        }
        gk.galois_key_generated_ = true;
    }

  private:
    HEContext<S> context_;
    hegpu_rng* rng_ = nullptr;
};

template <Scheme S> class HEEncryptor { // host/ckks/encryptor.cuh (public-key encryption)
  public:
    HEEncryptor(HEContext<S> context, Publickey<S>& pk) : context_(std::move(context)), pk_(&pk)
    {
        detail::require_generated(context_);
        if (!pk.public_key_generated_) throw std::logic_error("Publickey is not generated!");
        detail::check(hegpu_rng_create_from_entropy(&rng_));
    }
    // REPRODUCIBLE TESTS ONLY (64-bit seed)
    HEEncryptor(HEContext<S> context, Publickey<S>& pk, std::uint64_t seed) : context_(std::move(context)), pk_(&pk)
    {
        detail::require_generated(context_);
        if (!pk.public_key_generated_) throw std::logic_error("Publickey is not generated!");
        detail::check(hegpu_rng_create(seed, &rng_));
    }
    ~HEEncryptor() { hegpu_rng_destroy(rng_); }
    HEEncryptor(const HEEncryptor&) = delete;
    HEEncryptor& operator=(const HEEncryptor&) = delete;

    void encrypt(Ciphertext<S>& ct, Plaintext<S>& pt, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!pt.plaintext_generated_ || pt.depth_ != 0) throw std::invalid_argument("Invalid plaintext size."); // encryptor.cuh:56
        DeviceVector<Data64> out((size_t) 2 * context_->Q_size * context_->n, o.stream_);
        const int opid = (S == Scheme::CKKS) ? HEGPU_OP_CKKS_ENCRYPT : HEGPU_OP_BFV_ENCRYPT;
        detail::Workspace ws(context_->handle(), opid, 0, o.stream_);
        detail::check((S == Scheme::CKKS ? hegpu_ckks_encrypt : hegpu_bfv_encrypt)(
            context_->handle(), rng_, (const uint64_t*) pk_->data(), (const uint64_t*) pt.data(), (uint64_t*) out.data(),
            ws.data(), ws.bytes, o.stream_));
        ct.adopt(std::move(out), 2, 0, pt.scale_);
        ct.encoding_ = pt.encoding_; // ckks/encryptor.cuh:84
    }

  private:
    HEContext<S> context_;
    Publickey<S>* pk_;
    hegpu_rng* rng_ = nullptr;
};

template <Scheme S> class HEDecryptor { // host/ckks/decryptor.cuh
  public:
    HEDecryptor(HEContext<S> context, Secretkey<S>& sk) : context_(std::move(context)), sk_(&sk)
    {
        detail::require_generated(context_);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
    }
    void decrypt(Plaintext<S>& pt, Ciphertext<S>& ct, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (ct.size() != 2) throw std::invalid_argument("Ciphertext should be relinearized first!");
        const int l = context_->Q_size - ct.depth();
        DeviceVector<Data64> out((S == Scheme::CKKS) ? (size_t) l * context_->n : (size_t) context_->n, o.stream_);
        if (S == Scheme::CKKS) {
            detail::check(hegpu_ckks_decrypt(context_->handle(), (const uint64_t*) ct.data(),
                                             (const uint64_t*) sk_->data(), ct.depth(), (uint64_t*) out.data(),
                                             o.stream_));
        } else {
            detail::Workspace ws(context_->handle(), HEGPU_OP_BFV_DECRYPT, 0, o.stream_);
            detail::check(hegpu_bfv_decrypt(context_->handle(), (const uint64_t*) ct.data(),
                                            (const uint64_t*) sk_->data(), (uint64_t*) out.data(), ws.data(), ws.bytes,
                                            o.stream_));
        }
        pt.memory_set(std::move(out));
        pt.depth_ = ct.depth();
        pt.scale_ = ct.scale();
        pt.encoding_ = ct.encoding_; // ckks/decryptor.cuh:81
        pt.plaintext_generated_ = true;
    }

    // BFV invariant noise budget in bits: log2(Q) - log2(|t * (c0 + c1 s) mod Q|_inf) - 1
    // (bfv/decryptor.cu:170-300); the residues come from the device, the CRT composition and the
    // norm are done here on the host with multi-word integers
    int remainder_noise_budget(Ciphertext<S>& ct, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::BFV, "the noise budget is defined for BFV");
        const int Q = context_->Q_size;
        const size_t n = context_->n;
        DeviceVector<Data64> out((size_t) Q * n, o.stream_);
        detail::check(hegpu_bfv_noise_rns(context_->handle(), (const uint64_t*) ct.data(), (const uint64_t*) sk_->data(),
                                          (uint64_t*) out.data(), o.stream_));
        std::vector<Data64> h((size_t) Q * n);
        detail::hip(hipMemcpyAsync(h.data(), out.data(), h.size() * sizeof(Data64), hipMemcpyDeviceToHost, o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
        typedef unsigned __int128 u128;
        const std::vector<Data64> q = context_->get_key_modulus();
        auto mul_word = [](std::vector<Data64>& big, Data64 f) {
            u128 carry = 0;
            for (Data64& w : big) { u128 v = (u128) w * f + carry; w = (Data64) v; carry = v >> 64; }
            big.push_back((Data64) carry);
        };
        std::vector<Data64> M{1};
        for (int j = 0; j < Q; j++) mul_word(M, q[j]);
        M.resize(Q + 1, 0);
        std::vector<std::vector<Data64>> Mi(Q);
        std::vector<Data64> Mi_inv(Q);
        auto mulmod = [](Data64 a, Data64 b, Data64 m) { return (Data64) ((u128) a * b % m); };
        auto powmod = [&](Data64 a, Data64 e, Data64 m) { Data64 r = 1; while (e) { if (e & 1) r = mulmod(r, a, m); a = mulmod(a, a, m); e >>= 1; } return r; };
        for (int i = 0; i < Q; i++) {
            Mi[i] = {1};
            Data64 m = 1;
            for (int j = 0; j < Q; j++)
                if (j != i) { mul_word(Mi[i], q[j]); m = mulmod(m, q[j] % q[i], q[i]); }
            Mi[i].resize(Q + 1, 0);
            Mi_inv[i] = powmod(m, q[i] - 2, q[i]);
        }
        auto geq = [&](const std::vector<Data64>& a, const std::vector<Data64>& b) {
            for (int k = Q; k >= 0; k--) if (a[k] != b[k]) return a[k] > b[k];
            return true;
        };
        auto sub = [&](std::vector<Data64>& a, const std::vector<Data64>& b) {
            Data64 borrow = 0;
            for (int k = 0; k <= Q; k++) { u128 d = (u128) a[k] - b[k] - borrow; a[k] = (Data64) d; borrow = (Data64) (d >> 64) & 1; }
        };
        std::vector<Data64> half = M; // M >> 1
        for (int k = 0; k <= Q; k++) half[k] = (M[k] >> 1) | (k < Q ? (M[k + 1] << 63) : 0);
        auto bit_length = [&](const std::vector<Data64>& a) {
            for (int k = Q; k >= 0; k--) if (a[k]) { int b = 0; Data64 v = a[k]; while (v) { b++; v >>= 1; } return 64 * k + b; }
            return 0;
        };
        int norm_bits = 0;
        std::vector<Data64> acc(Q + 1), term(Q + 1);
        for (size_t c = 0; c < n; c++) {
            std::fill(acc.begin(), acc.end(), 0);
            for (int i = 0; i < Q; i++) {
                const Data64 t = mulmod(h[(size_t) i * n + c], Mi_inv[i], q[i]);
                u128 carry = 0;
                for (int k = 0; k <= Q; k++) { u128 v = (u128) Mi[i][k] * t + acc[k] + carry; acc[k] = (Data64) v; carry = v >> 64; }
                if (geq(acc, M)) sub(acc, M);
            }
            if (geq(acc, half)) { term = M; sub(term, acc); norm_bits = std::max(norm_bits, bit_length(term)); }
            else norm_bits = std::max(norm_bits, bit_length(acc));
        }
        const int budget = bit_length(M) - norm_bits - 1;
        return budget < 0 ? 0 : budget;
    }

  private:
    HEContext<S> context_;
    Secretkey<S>* sk_;
};

// ------------------------------------------------------------------ encoders
template <Scheme S> class HEEncoder;

template <> class HEEncoder<Scheme::BFV> { // host/bfv/encoder.cuh: batching over the slots of Z_t[X]/(X^N+1)
    static constexpr Scheme S = Scheme::BFV;

  public:
    explicit HEEncoder(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
    inline int slot_count() const noexcept { return context_->n; }

    // messages in pinned host memory (HostVector, util/hostvector.cuh; benchmark_bfv.cpp:49,170)
    template <typename T> void encode(Plaintext<S>& plain, const HostVector<T>& message, const ExecutionOptions& o = ExecutionOptions())
    {
        encode(plain, std::vector<T>(message.begin(), message.end()), o);
    }
    template <typename T> void decode(HostVector<T>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        std::vector<T> m;
        decode(m, plain, o);
        message.assign(m.begin(), m.end());
    }
    void encode(Plaintext<S>& plain, const std::vector<int64_t>& message, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if ((int) message.size() > context_->n)
            throw std::invalid_argument("Message size can not be higher than the slot count."); // bfv/encoder.cuh:60
        DeviceVector<Data64> msg(message.size() ? message.size() : 1, o.stream_);
        if (!message.empty())
            detail::hip(hipMemcpyAsync(msg.data(), message.data(), message.size() * sizeof(int64_t),
                                       hipMemcpyHostToDevice, o.stream_));
        DeviceVector<Data64> out((size_t) context_->n, o.stream_);
        detail::check(hegpu_bfv_encode(context_->handle(), (const int64_t*) msg.data(), (int) message.size(),
                                       (uint64_t*) out.data(), o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_)); // `message` may be a temporary
        plain.memory_set(std::move(out));
        plain.depth_ = 0;
        plain.plaintext_generated_ = true;
    }
    void encode(Plaintext<S>& plain, const std::vector<uint64_t>& message, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        std::vector<int64_t> m(message.begin(), message.end());
        encode(plain, m, o);
    }
    void decode(std::vector<uint64_t>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        DeviceVector<Data64> out((size_t) context_->n, o.stream_), ws((size_t) context_->n, o.stream_);
        detail::check(hegpu_bfv_decode(context_->handle(), (const uint64_t*) plain.data(), (uint64_t*) out.data(),
                                       ws.data(), ws.size() * sizeof(Data64), o.stream_));
        message.resize(context_->n);
        detail::hip(hipMemcpyAsync(message.data(), out.data(), message.size() * sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
    }
    void decode(std::vector<int64_t>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        std::vector<uint64_t> u;
        decode(u, plain, o);
        const uint64_t t = context_->get_plain_modulus();
        message.resize(u.size());
        for (size_t i = 0; i < u.size(); i++) // centred representative
            message[i] = u[i] > (t >> 1) ? (int64_t) u[i] - (int64_t) t : (int64_t) u[i];
    }

  private:
    HEContext<S> context_;
};

template <> class HEEncoder<Scheme::CKKS> { // host/ckks/encoder.cuh: N/2 complex slots or N coefficients
    static constexpr Scheme S = Scheme::CKKS;

  public:
    explicit HEEncoder(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
    inline int slot_count() const noexcept { return context_->n >> 1; }

    // real vector into the slots, or (encoding::COEFFICIENT) as the polynomial itself (encoder.cuh:56-115)
    // messages in pinned host memory (HostVector, util/hostvector.cuh; benchmark_ckks.cpp:64,186)
    template <typename T> void encode(Plaintext<S>& plain, const HostVector<T>& message, double scale,
                                      const ExecutionOptions& o = ExecutionOptions())
    {
        // Round 6: NO copy at all.  hipHostMalloc memory is mapped into the device's address space, and since round 6 the
        // special FFT converts the message in its first load (encode.hip: en_load): the transform reads the 8 N / 2 bytes
        // straight out of the pinned vector over the host link.  (Rounds 2-5 went through a pageable copy -- 78 us against
        // 150 us for a DMA copy of the pinned source at N = 4096; the upload was ~16 us of a 0.09 ms call.)
        encode_from(plain, message, scale, o, encoding::SLOT, true);
    }
    // decoded straight into the pinned vector: the transform's last store writes the message there, no copy (same-box
    // A/B against the DMA copy of rounds 2-5, benchmark_ckks.cpp decode: N = 2^12..2^15 0.060 / 0.074 / 0.108 / 0.197 ms against
    // 0.071 / 0.100 / 0.130 / 0.224 -- profiles/r6_experiments/encode_decode_mapped_ab.txt)
    template <typename T> void decode(HostVector<T>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        decode_to(message, plain, o, true);
    }
    void encode(Plaintext<S>& plain, const std::vector<double>& message, double scale,
                const ExecutionOptions& o = ExecutionOptions(), encoding type = encoding::SLOT)
    {
        encode_from(plain, message, scale, o, type);
    }
    // complex vector into the slots (encoder.cuh:188-235)
    void encode(Plaintext<S>& plain, const std::vector<Complex64>& message, double scale,
                const ExecutionOptions& o = ExecutionOptions())
    {
        encode_from(plain, message, scale, o);
    }

  private:
    // `mapped`: the vector lives in pinned, device-visible memory (HostVector): the kernels read it where it is
    template <typename A> void encode_from(Plaintext<S>& plain, const std::vector<double, A>& message, double scale,
                                           const ExecutionOptions& o, encoding type = encoding::SLOT, bool mapped = false)
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        check_scale(scale);
        if (type == encoding::SLOT && (int) message.size() > slot_count())
            throw std::invalid_argument("Vector size can not be higher than slot count!");        // :74
        if (type != encoding::SLOT && message.size() > (size_t) context_->n)
            throw std::invalid_argument("Vector size can not be higher than polynomial degree!"); // :80
        mapped = mapped && !message.empty();
        DeviceVector<Data64> msg(mapped ? 1 : (message.size() ? message.size() : 1), o.stream_);
        if (!mapped && !message.empty())
            detail::hip(hipMemcpyAsync(msg.data(), message.data(), message.size() * sizeof(double),
                                       hipMemcpyHostToDevice, o.stream_));
        const double* src = mapped ? message.data() : (const double*) msg.data();
        DeviceVector<Data64> out((size_t) context_->Q_size * context_->n, o.stream_);
        if (type == encoding::SLOT) {
            detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_ENCODE, 0, o.stream_);
            detail::check(hegpu_ckks_encode(context_->handle(), src, (int) message.size(), scale,
                                            (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
        } else {
            detail::check(hegpu_ckks_encode_coeff(context_->handle(), src, (int) message.size(),
                                                  scale, (uint64_t*) out.data(), o.stream_));
        }
        finish(plain, std::move(out), scale, type, o); // (synchronises: the caller may change `message` afterwards)
    }
    template <typename A> void encode_from(Plaintext<S>& plain, const std::vector<Complex64, A>& message, double scale,
                                           const ExecutionOptions& o, encoding = encoding::SLOT, bool mapped = false)
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        check_scale(scale);
        if ((int) message.size() > slot_count())
            throw std::invalid_argument("Vector size can not be higher than slot count!");
        mapped = mapped && !message.empty();
        DeviceVector<Data64> msg(mapped ? 1 : (message.size() ? 2 * message.size() : 1), o.stream_);
        if (!mapped && !message.empty())
            detail::hip(hipMemcpyAsync(msg.data(), message.data(), message.size() * sizeof(Complex64),
                                       hipMemcpyHostToDevice, o.stream_));
        const double* src = mapped ? (const double*) message.data() : (const double*) msg.data();
        DeviceVector<Data64> out((size_t) context_->Q_size * context_->n, o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_ENCODE, 0, o.stream_);
        detail::check(hegpu_ckks_encode_complex(context_->handle(), src, (int) message.size(), scale,
                                                (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
        finish(plain, std::move(out), scale, encoding::SLOT, o);
    }

  public:
    // one number in every slot (encoder.cuh:290-370)
    void encode(Plaintext<S>& plain, const double& message, double scale, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        check_scale(scale);
        DeviceVector<Data64> out((size_t) context_->Q_size * context_->n, o.stream_);
        detail::check(hegpu_ckks_encode_scalar(context_->handle(), message, scale, (uint64_t*) out.data(), o.stream_));
        finish(plain, std::move(out), scale, encoding::SLOT, o);
    }
    void encode(Plaintext<S>& plain, const std::int64_t& message, double scale,
                const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        encode(plain, static_cast<double>(message), scale, o); // encoder.cu:437
    }

    void decode(std::vector<double>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        decode_to(message, plain, o);
    }
    void decode(std::vector<Complex64>& message, Plaintext<S>& plain, const ExecutionOptions& o = ExecutionOptions())
    {
        decode_to(message, plain, o);
    }

  private:
    template <typename A> void decode_to(std::vector<double, A>& message, Plaintext<S>& plain, const ExecutionOptions& o,
                                         bool mapped = false)
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        const bool coeff = plain.encoding_ == encoding::COEFFICIENT; // encoder.cuh:383
        const size_t count = coeff ? (size_t) context_->n : (size_t) slot_count();
        message.resize(count);
        DeviceVector<Data64> out(mapped ? 1 : count, o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_DECODE, plain.depth_, o.stream_);
        detail::check((coeff ? hegpu_ckks_decode_coeff : hegpu_ckks_decode)(
            context_->handle(), (const uint64_t*) plain.data(), plain.depth_, plain.scale_,
            mapped ? message.data() : (double*) out.data(), ws.data(), ws.bytes, o.stream_));
        if (!mapped)
            detail::hip(hipMemcpyAsync(message.data(), out.data(), count * sizeof(double), hipMemcpyDeviceToHost, o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
    }
    template <typename A> void decode_to(std::vector<Complex64, A>& message, Plaintext<S>& plain, const ExecutionOptions& o,
                                         bool mapped = false)
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (plain.encoding_ == encoding::COEFFICIENT)
            throw std::invalid_argument("Coefficient encoded CKKS plaintext can not be decoded to complex slots."); // :438
        message.resize(slot_count());
        DeviceVector<Data64> out(mapped ? 1 : (size_t) 2 * slot_count(), o.stream_);
        detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_DECODE, plain.depth_, o.stream_);
        detail::check(hegpu_ckks_decode_complex(context_->handle(), (const uint64_t*) plain.data(), plain.depth_,
                                                plain.scale_, mapped ? (double*) message.data() : (double*) out.data(),
                                                ws.data(), ws.bytes, o.stream_));
        if (!mapped)
            detail::hip(hipMemcpyAsync(message.data(), out.data(), message.size() * sizeof(Complex64), hipMemcpyDeviceToHost,
                                       o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
    }

  private:
    void check_scale(double scale) const // encoder.cuh:60-65
    {
        if (scale <= 0 || static_cast<int>(std::log2(scale)) >= context_->total_coeff_bit_count)
            throw std::invalid_argument("Scale out of bounds");
    }
    void finish(Plaintext<S>& plain, DeviceVector<Data64>&& out, double scale, encoding type, const ExecutionOptions& o)
    {
        detail::hip(hipStreamSynchronize(o.stream_)); // the staging buffer of the message dies with the caller
        plain.memory_set(std::move(out));
        plain.depth_ = 0;
        plain.scale_ = scale;
        plain.encoding_ = type;
        plain.plaintext_generated_ = true;
    }
    HEContext<S> context_;
};

// ------------------------------------------------------------------ plaintext matrix for HEArithmeticOperator::linear_transform
// A matrix M over the N/2 slots, given by its non-zero diagonals diag_k[s] = M[s][(s + k) mod N/2], prepared for the
// baby-step/giant-step evaluation of y = M v (hegpu_ckks_linear_transform).  This is the project's own addition: the
// reference's multiply_matrix (ckks/operator.cu:2803-2895) is private to its bootstrapping and takes pre-baked index
// tensors.  The plan (the same as heongpu_amd.api.linear_transform_plan): with the baby-step period n1, diagonal
// k = j n1 + i is baby step i of giant step j; only the i and j that occur are kept; the slot vector of diagonal k is
// rotated by -j n1 before it is encoded, so that rot(j n1, diag' * rot(i, v)) = diag_k * rot(k, v).  With a stride (a
// group of FFT stages: every diagonal index is a multiple of it) the plan is made over k / stride: k = stride (j n1 + i),
// baby shifts stride i, giant shifts stride j n1.
// chain_giant_steps: the giant steps are chained (hegpu_giant_step_chain, hegpu_ckks_linear_transform_chained): each inner
// sum is folded into its neighbour nearer zero and travels over the differences of neighbouring giant shifts.  The
// diagonals, the number of key switches and the result's meaning are those of the direct mode; required_shifts() holds
// the links in the place of the giant shifts -- for giant steps that are dense around zero two keys, not n2 - 1.
template <Scheme S> class LinearTransform;
template <> class LinearTransform<Scheme::CKKS> {
    static constexpr Scheme S = Scheme::CKKS;

  public:
    // n1: the baby-step period; 0 = the power of two nearest the square root of the number of diagonals (the larger one
    // on a tie), at most 16.  Diagonals shorter than N/2 are padded with zeros.
    LinearTransform(HEContext<S> context, const std::map<int, std::vector<Complex64>>& diagonals, HEEncoder<S>& encoder,
                    double scale, int depth = 0, int n1 = 0, const ExecutionOptions& o = ExecutionOptions(), int stride = 1,
                    bool chain_giant_steps = false)
        : context_(std::move(context))
    {
        build(diagonals, encoder, scale, depth, n1, o, stride, chain_giant_steps);
    }
    LinearTransform(HEContext<S> context, const std::map<int, std::vector<double>>& diagonals, HEEncoder<S>& encoder,
                    double scale, int depth = 0, int n1 = 0, const ExecutionOptions& o = ExecutionOptions(), int stride = 1,
                    bool chain_giant_steps = false)
        : context_(std::move(context))
    {
        build(diagonals, encoder, scale, depth, n1, o, stride, chain_giant_steps);
    }
    // the rotations linear_transform needs a Galois key of their own for (no power-of-two chains there): the baby shifts
    // and the giant shifts, with chain_giant_steps the links of the chain in their place
    std::vector<int> required_shifts() const
    {
        std::vector<int> v;
        for (int sh : baby_shifts_) if (sh) v.push_back(sh);
        for (int sh : link_shifts()) if (sh && std::find(v.begin(), v.end(), sh) == v.end()) v.push_back(sh);
        return v;
    }
    bool chained() const noexcept { return !giant_parent_.empty(); }
    // per giant step the rotation linear_transform applies to it: its own shift, or with chain_giant_steps its link
    const std::vector<int>& link_shifts() const noexcept { return chained() ? link_shifts_ : giant_shifts_; }
    // hegpu_ckks_linear_transform_chained's giant_parent: nullptr = direct
    const int* giant_parent() const noexcept { return chained() ? giant_parent_.data() : nullptr; }
    double scale() const noexcept { return scale_; }
    int depth() const noexcept { return depth_; }
    int n1() const noexcept { return (int) baby_shifts_.size(); }
    int n2() const noexcept { return (int) giant_shifts_.size(); }
    int diagonal_count() const noexcept { return n_diag_; }
    const std::vector<int>& index() const noexcept { return index_; }            // [n2][n1], -1 = no such diagonal
    const std::vector<int>& baby_shifts() const noexcept { return baby_shifts_; }
    const std::vector<int>& giant_shifts() const noexcept { return giant_shifts_; }
    const Data64* data() const { return diags_.data(); }                          // [diagonal_count][Q - depth][N]

  private:
    template <typename T> void build(const std::map<int, std::vector<T>>& diagonals, HEEncoder<S>& encoder, double scale,
                                     int depth, int n1, const ExecutionOptions& o, int stride, bool chain_giant_steps)
    {
        detail::require_generated(context_);
        if (depth < 0 || depth >= context_->Q_size) throw std::invalid_argument("Invalid depth!");
        if (stride < 1) throw std::invalid_argument("The stride is at least 1!");
        const int slots = (int) (context_->n >> 1);
        std::map<int, const std::vector<T>*> by_k; // diagonal index mod slots, ascending
        for (const auto& d : diagonals) {
            if ((int) d.second.size() > slots) throw std::invalid_argument("Vector size can not be higher than slot count!");
            if (!by_k.emplace(((d.first % slots) + slots) % slots, &d.second).second)
                throw std::invalid_argument("Two diagonals with the same index modulo the slot count!");
        }
        if (by_k.empty()) throw std::invalid_argument("A linear transform needs at least one diagonal!");
        for (const auto& d : by_k)
            if (d.first % stride) throw std::invalid_argument("Every diagonal index is a multiple of the stride!");
        if (n1 == 0) {
            const double root = std::sqrt((double) by_k.size());
            n1 = 1;
            for (int p2 = 2; p2 <= 16; p2 *= 2)
                if (std::fabs(p2 - root) <= std::fabs(n1 - root)) n1 = p2;
        }
        if (n1 < 1 || n1 > 16) throw std::invalid_argument("The baby-step period lies in [1, 16]!");
        std::vector<int> babies, giants;
        for (const auto& d : by_k) {
            const int q = d.first / stride;
            if (std::find(babies.begin(), babies.end(), q % n1) == babies.end()) babies.push_back(q % n1);
            if (std::find(giants.begin(), giants.end(), q / n1) == giants.end()) giants.push_back(q / n1);
        }
        std::sort(babies.begin(), babies.end());
        std::sort(giants.begin(), giants.end());
        if (giants.size() > 16)
            throw std::invalid_argument("More than 16 giant steps: choose a larger baby-step period!");
        index_.assign(babies.size() * giants.size(), -1);
        scale_ = scale;
        depth_ = depth;
        n_diag_ = (int) by_k.size();
        const size_t n = context_->n, l = (size_t) (context_->Q_size - depth);
        diags_ = DeviceVector<Data64>((size_t) n_diag_ * l * n, o.stream_);
        int pos = 0;
        for (const auto& d : by_k) {
            const int i = (d.first / stride) % n1, j = (d.first / stride) / n1;
            const size_t row = std::find(giants.begin(), giants.end(), j) - giants.begin();
            const size_t col = std::find(babies.begin(), babies.end(), i) - babies.begin();
            index_[row * babies.size() + col] = pos;
            std::vector<T> rotated((size_t) slots, T(0)); // rotated by -stride j n1: slot t takes slot t - stride j n1
            for (size_t t = 0; t < d.second->size(); t++)
                rotated[(t + (size_t) stride * j * n1) % slots] = (*d.second)[t];
            Plaintext<S> plain(context_);
            encoder.encode(plain, rotated, scale, o);
            detail::hip(hipMemcpyAsync(diags_.data() + (size_t) pos * l * n, plain.data(), l * n * sizeof(Data64),
                                       hipMemcpyDeviceToDevice, o.stream_));
            detail::hip(hipStreamSynchronize(o.stream_)); // `plain` is released at the end of this iteration
            pos++;
        }
        baby_shifts_.clear();
        giant_shifts_.clear();
        for (int i : babies) baby_shifts_.push_back(stride * i);
        for (int j : giants) giant_shifts_.push_back(stride * j * n1);
        giant_parent_.clear();
        link_shifts_.clear();
        if (chain_giant_steps) {
            giant_parent_.resize(giant_shifts_.size());
            link_shifts_.resize(giant_shifts_.size());
            detail::check(hegpu_giant_step_chain(giant_shifts_.data(), (int) giant_shifts_.size(), slots, giant_parent_.data(),
                                                 link_shifts_.data()));
        }
    }
    HEContext<S> context_;
    DeviceVector<Data64> diags_;
    std::vector<int> index_, baby_shifts_, giant_shifts_, giant_parent_, link_shifts_;
    double scale_ = 0;
    int depth_ = 0, n_diag_ = 0;
};

// ------------------------------------------------------------------ polynomials evaluated on ciphertexts
// host/ckks/operator.cuh:1902-1937 (there a class nested in HEOperator<CKKS>) and PolyType.  coeffs_[i] multiplies x^i
// (MONOMIAL) or T_i(x), x in [-1, 1] (CHEBYSHEV); max_deg_ / lead_ steer the split of evaluate_poly as in the reference
// (a polynomial of its own: max_deg = its degree, lead = true); a_ / b_ record the interval a caller mapped to [-1, 1].
enum class PolyType { MONOMIAL, CHEBYSHEV };
class Polynomial {
  public:
    Polynomial() : type_(PolyType::CHEBYSHEV), max_deg_(0), lead_(false), a_(0.0), b_(0.0) {}
    Polynomial(int max_deg, const std::vector<Complex64>& coeffs, bool lead = false, PolyType type = PolyType::CHEBYSHEV,
               double a = 0.0, double b = 0.0)
        : type_(type), max_deg_(max_deg), coeffs_(coeffs), lead_(lead), a_(a), b_(b)
    {
    }
    int degree() const { return (int) coeffs_.size() - 1; }
    // ceil(log2(degree + 1)), the bit length of the degree: the levels evaluate_poly spends.  The reference's depth() is
    // ceil(log2(degree)); the two differ for a degree that is a power of two only, where the reference's first split reads a
    // power it never made (the plan's first departure, hegpu.h)
    int depth() const { return (int) std::ceil(std::log2((double) coeffs_.size())); }
    PolyType type_;
    int max_deg_;
    std::vector<Complex64> coeffs_;
    bool lead_;
    double a_, b_;
};

// ------------------------------------------------------------------ CoeffToSlot / SlotToCoeff context
// host/ckks/operator.cuh:29-82.  The reference keeps pre-baked index tensors of its Vandermonde generator; here the
// factors are LinearTransform objects over the groups of hegpu_encoding_transform_shape / _fill.
struct CKKSEncodingTransformConfig {
    int CtoS_piece_;       // [2, 5]
    int StoC_piece_;       // [2, 5]
    int CtoS_start_level_; // ciphertext level where CoeffToSlot starts
    int StoC_start_level_; // ciphertext level where SlotToCoeff starts
    bool less_key_mode_;   // the reference's own key chain: refused (HEArithmeticOperator::set_chained_giant_steps is this
                           // backend's reduced key set)
    CKKSEncodingTransformConfig(int CtoS_piece = 3, int StoC_piece = 3, bool less_key_mode = true)
        : CtoS_piece_(CtoS_piece), StoC_piece_(StoC_piece), CtoS_start_level_(-1), StoC_start_level_(-1),
          less_key_mode_(less_key_mode)
    {
    }
    CKKSEncodingTransformConfig(int CtoS_piece, int StoC_piece, int CtoS_start_level, int StoC_start_level,
                                bool less_key_mode = true)
        : CtoS_piece_(CtoS_piece), StoC_piece_(StoC_piece), CtoS_start_level_(CtoS_start_level),
          StoC_start_level_(StoC_start_level), less_key_mode_(less_key_mode)
    {
    }
};
struct CKKSEncodingTransformContext {
    bool generated_ = false;
    bool less_key_mode_ = false;
    double scale_boot_ = 0.0;
    int CtoS_piece_ = 0;
    int StoC_piece_ = 0;
    int CtoS_level_ = 0;
    int StoC_level_ = 0;
    std::vector<int> key_indexs_; // every rotation of every factor: Galoiskey(context, key_indexs_) is enough
    // the factors in the order they are applied; factor k of CtoS is encoded at CtoS_level_ + k, of StoC at
    // StoC_level_ + 1 + k
    std::vector<std::shared_ptr<LinearTransform<Scheme::CKKS>>> CtoS_factors_, StoC_factors_;
};

// ------------------------------------------------------------------ configuration of the CKKS refresh
// util/util.cuh:60-202: the names, fields and defaults of the reference.  level_start_ is a level (the index of a
// ciphertext's last prime).  Read by HEArithmeticOperator<CKKS>::generate_bootstrapping_params_v2: Q_,
// scaling_factor_, arcsine_deg_, sqrt2pi_, q_diff_ and bsgs_ratio_ are carried for the reference's callers and not used --
// scales are exact labels here, the baby-step period is the linear transform's own rule.
enum class SineType { COS1 };
enum class LinearTransformType { COEFFS_TO_SLOTS, SLOTS_TO_COEFFS };
struct EvalModConfig {
    Data64 Q_ = 0;
    int level_start_ = 0;
    double message_ratio_ = 0.0;
    int K_ = 0;
    int sine_deg_ = 0;
    int double_angle_ = 0;
    int arcsine_deg_ = 0;
    double scaling_factor_ = 0.0;
    int piece_ = 0;
    double sqrt2pi_ = 0.0;
    double q_diff_ = 0.0;
    SineType sine_type_ = SineType::COS1;
    PolyType poly_type_ = PolyType::CHEBYSHEV;
    EvalModConfig() {}
    EvalModConfig(int level_start) : level_start_(level_start), message_ratio_(256.0), K_(16), sine_deg_(30), double_angle_(3) {}
    EvalModConfig(Data64 Q, int level_start, double message_ratio, int K, int sine_deg, int double_angle, int arcsine_deg,
                  double scaling_factor)
        : Q_(Q), level_start_(level_start), message_ratio_(message_ratio), K_(K), sine_deg_(sine_deg),
          double_angle_(double_angle), arcsine_deg_(arcsine_deg), scaling_factor_(scaling_factor)
    {
        if (Q != 0) q_diff_ = (double) Q / std::exp2(std::round(std::log2((double) Q)));
        if (Q != 0 && scaling_factor != 0.0)
            sqrt2pi_ = std::pow((double) Q * 0.5 / (scaling_factor * 3.14159265358979323846), 1.0 / std::exp2((double) double_angle));
    }
};
struct EncodingMatrixConfig {
    LinearTransformType lt_type_ = LinearTransformType::COEFFS_TO_SLOTS;
    int level_start_ = 0;
    double bsgs_ratio_ = 0.0;
    int piece_ = 0;
    EncodingMatrixConfig() {}
    EncodingMatrixConfig(LinearTransformType lt_type, int level_start) : EncodingMatrixConfig(lt_type, level_start, 2.0) {}
    EncodingMatrixConfig(LinearTransformType lt_type, int level_start, double bsgs_ratio)
        : EncodingMatrixConfig(lt_type, level_start, bsgs_ratio, lt_type == LinearTransformType::COEFFS_TO_SLOTS ? 4 : 3)
    {
    }
    EncodingMatrixConfig(LinearTransformType lt_type, int level_start, double bsgs_ratio, int piece)
        : lt_type_(lt_type), level_start_(level_start), bsgs_ratio_(bsgs_ratio), piece_(piece)
    {
    }
};
struct BootstrappingConfigV2 {
    int CtoS_piece_;
    int StoC_piece_;
    EncodingMatrixConfig cts_config_;
    EncodingMatrixConfig stc_config_;
    EvalModConfig eval_mod_config_;
    BootstrappingConfigV2(EncodingMatrixConfig stc_config, EvalModConfig eval_mod_config, EncodingMatrixConfig cts_config)
        : CtoS_piece_(cts_config.piece_), StoC_piece_(stc_config.piece_), cts_config_(cts_config), stc_config_(stc_config),
          eval_mod_config_(eval_mod_config)
    {
    }
};

// util/util.cuh:176-188, util/schemes.h:113-127: the configuration and the kinds of the reference's first bootstrapping
// family.  Here slim, bit and gate bootstrapping run on the parts of the regular refresh: taylor_number_
// and less_key_mode_ are validated and carried as the reference does, and not used -- EvalMod is the Chebyshev cosine
// with K = 12, degree 30 and three double angles, and the rotations are the linear transforms' own.
struct BootstrappingConfig {
    int CtoS_piece_;      // Default: 3
    int StoC_piece_;      // Default: 3
    int taylor_number_;   // Default: 11
    bool less_key_mode_;  // Default: false; carried, unused (the reduced key set: set_chained_giant_steps)
    BootstrappingConfig(int CtoS = 3, int StoC = 3, int taylor = 11, bool less_key_mode = false)
        : CtoS_piece_(CtoS), StoC_piece_(StoC), taylor_number_(taylor), less_key_mode_(less_key_mode)
    {
        if (CtoS_piece_ < 2 || CtoS_piece_ > 5) throw std::out_of_range("CtoS_piece must be in range [2, 5]");
        if (StoC_piece_ < 2 || StoC_piece_ > 5) throw std::out_of_range("StoC_piece must be in range [2, 5]");
        if (taylor_number_ < 6 || taylor_number_ > 15) throw std::out_of_range("taylor_number must be in range [6, 15]");
    }
};
enum class arithmetic_bootstrapping_type : std::uint8_t { NONE = 0x0, REGULAR_BOOTSTRAPPING = 0x1, SLIM_BOOTSTRAPPING = 0x2 };
enum class logic_bootstrapping_type : std::uint8_t {
    NONE = 0x0,
    BIT_BOOTSTRAPPING = 0x1,  // scale = q0 / 2 (eprint 2024/767)
    GATE_BOOTSTRAPPING = 0x2, // scale = q0 / 3
};

// ------------------------------------------------------------------ precision of decoded CKKS values
// host/ckks/precision.cuh: per slot the distance of the real parts, of the imaginary parts and of the complex numbers
// (l2); precision = log2(1 / delta).  The distributions (cdf_resol steps of 0.01 bit up to the best precision seen) count
// the slots whose precision is at least that step.
struct Stats {
    double real, imag, l2;
    Stats() : real(0.0), imag(0.0), l2(0.0) {}
    Stats(double r, double i, double l2_val) : real(r), imag(i), l2(l2_val) {}
};
struct DistEntry {
    double prec;
    int count;
    DistEntry() : prec(0.0), count(0) {}
};
inline Stats delta_to_precision(const Stats& d) { return Stats(std::log2(1.0 / d.real), std::log2(1.0 / d.imag), std::log2(1.0 / d.l2)); }
inline Stats calc_median(std::vector<Stats>& values)
{
    if (values.empty()) return Stats();
    std::vector<double> r, i, l;
    for (const Stats& s : values) { r.push_back(s.real); i.push_back(s.imag); l.push_back(s.l2); }
    auto mid = [](std::vector<double>& v) {
        std::sort(v.begin(), v.end());
        const size_t h = v.size() / 2;
        return v.size() % 2 ? v[h] : 0.5 * (v[h - 1] + v[h]);
    };
    return Stats(mid(r), mid(i), mid(l));
}
inline void calc_cdf(const std::vector<double>& precs, std::vector<DistEntry>& res, int cdf_resol)
{
    res.assign((size_t) (cdf_resol > 0 ? cdf_resol : 0), DistEntry());
    if (precs.empty() || cdf_resol < 1) return;
    std::vector<double> sorted(precs);
    std::sort(sorted.begin(), sorted.end());
    const double lo = sorted.front(), hi = sorted.back();
    for (int k = 0; k < cdf_resol; k++) {
        const double p = lo + (hi - lo) * k / (double) cdf_resol;
        res[(size_t) k].prec = p;
        res[(size_t) k].count = (int) (sorted.end() - std::lower_bound(sorted.begin(), sorted.end(), p));
    }
}
struct PrecisionStats {
    Stats max_delta, min_delta, max_precision, min_precision, mean_delta, mean_precision, median_delta, median_precision;
    std::vector<DistEntry> real_dist, imag_dist, l2_dist;
    int cdf_resol;
    PrecisionStats() : min_delta(1.0, 1.0, 1.0), cdf_resol(500) {}
    std::string to_string() const
    {
        std::ostringstream os;
        os << std::fixed << std::setprecision(2);
        auto row = [&](const char* name, const Stats& s) {
            os << name << " (real / imag / l2): " << s.real << " / " << s.imag << " / " << s.l2 << " bits\n";
        };
        row("MIN precision", min_precision);
        row("MAX precision", max_precision);
        row("AVG precision", mean_precision);
        row("MED precision", median_precision);
        os << std::scientific << "MAX delta (real / imag / l2): " << max_delta.real << " / " << max_delta.imag << " / "
           << max_delta.l2 << "\n";
        return os.str();
    }
};
inline PrecisionStats get_precision_stats(const std::vector<Complex64>& values_want, const std::vector<Complex64>& values_test)
{
    PrecisionStats p;
    const size_t slots = values_want.size() < values_test.size() ? values_want.size() : values_test.size();
    if (slots == 0) return p;
    std::vector<Stats> deltas(slots);
    std::vector<double> pr(slots), pi(slots), pl(slots);
    const double floor_delta = std::exp2(-1000.0); // an exact value has no finite precision: it counts as 1000 bits
    for (size_t k = 0; k < slots; k++) {
        const Complex64 d = values_test[k] - values_want[k];
        Stats s(std::fabs(d.real()), std::fabs(d.imag()), std::abs(d));
        for (double* v : {&s.real, &s.imag, &s.l2}) if (*v < floor_delta) *v = floor_delta;
        deltas[k] = s;
        p.mean_delta.real += s.real; p.mean_delta.imag += s.imag; p.mean_delta.l2 += s.l2;
        if (k == 0) p.max_delta = p.min_delta = s;
        p.max_delta = Stats(std::max(p.max_delta.real, s.real), std::max(p.max_delta.imag, s.imag), std::max(p.max_delta.l2, s.l2));
        p.min_delta = Stats(std::min(p.min_delta.real, s.real), std::min(p.min_delta.imag, s.imag), std::min(p.min_delta.l2, s.l2));
        const Stats b = delta_to_precision(s);
        pr[k] = b.real; pi[k] = b.imag; pl[k] = b.l2;
    }
    p.mean_delta = Stats(p.mean_delta.real / slots, p.mean_delta.imag / slots, p.mean_delta.l2 / slots);
    p.min_precision = delta_to_precision(p.max_delta);
    p.max_precision = delta_to_precision(p.min_delta);
    p.mean_precision = delta_to_precision(p.mean_delta);
    p.median_delta = calc_median(deltas);
    p.median_precision = delta_to_precision(p.median_delta);
    calc_cdf(pr, p.real_dist, p.cdf_resol);
    calc_cdf(pi, p.imag_dist, p.cdf_resol);
    calc_cdf(pl, p.l2_dist, p.cdf_resol);
    return p;
}
inline PrecisionStats get_precision_stats(const std::vector<double>& values_want, const std::vector<Complex64>& values_test)
{
    return get_precision_stats(std::vector<Complex64>(values_want.begin(), values_want.end()), values_test);
}
inline PrecisionStats get_precision_stats(const std::vector<double>& values_want, const std::vector<double>& values_test)
{
    return get_precision_stats(std::vector<Complex64>(values_want.begin(), values_want.end()),
                               std::vector<Complex64>(values_test.begin(), values_test.end()));
}

// ------------------------------------------------------------------ operator
template <Scheme S> class HEArithmeticOperator { // host/{bfv,ckks}/operator.cuh
    friend class detail::LogicOperatorBase<S>; // emit, require_words

  public:
    explicit HEArithmeticOperator(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
    // the reference's constructor takes the encoder (operator.cuh: used by its bootstrapping code only)
    HEArithmeticOperator(HEContext<S> context, HEEncoder<S>&) : HEArithmeticOperator(std::move(context)) {}

    void add(Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        binary(a, b, out, 0, o);
    }
    void sub(Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        binary(a, b, out, 1, o);
    }
    void negate(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        const int l = limbs(a);
        DeviceVector<Data64> m((size_t) a.cipher_size_ * l * context_->n, o.stream_);
        detail::check(hegpu_addition(context_->handle(), (const uint64_t*) a.data(), nullptr, (uint64_t*) m.data(), l,
                                     a.cipher_size_, 1, 2, o.stream_));
        emit(a, out, std::move(m));
    }

    // host/ckks/operator.cuh:632-689, host/bfv/operator.cuh:348-391
    void multiply(Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (a.relinearization_required_ || b.relinearization_required_)
            throw std::invalid_argument("Ciphertexts can not be multiplied because of the non-linear part! Please "
                                        "use relinearization operation!");
        if (a.rescale_required_ || b.rescale_required_)
            throw std::invalid_argument("Ciphertexts can not be multiplied because of the noise! Please use rescale "
                                        "operation to get rid of additional noise!");
        if (a.depth_ != b.depth_) throw std::logic_error("Ciphertexts leveled are not equal");
        const int l = limbs(a);
        const size_t n = context_->n;
        require_words(context_, a, 2);
        require_words(context_, b, 2);
        DeviceVector<Data64> m(3 * n * l, o.stream_);
        if (S == Scheme::CKKS) {
            detail::check(hegpu_ckks_multiply(context_->handle(), (const uint64_t*) a.data(), 0,
                                              (const uint64_t*) b.data(), 0, (uint64_t*) m.data(), 0, a.depth_, 1,
                                              o.stream_));
        } else {
            detail::Workspace ws(context_->handle(), HEGPU_OP_BFV_MULTIPLY, 0, o.stream_);
            detail::check(hegpu_bfv_multiply(context_->handle(), (const uint64_t*) a.data(), 0,
                                             (const uint64_t*) b.data(), 0, (uint64_t*) m.data(), 0, 1, ws.data(),
                                             ws.bytes, o.stream_));
        }
        const double sc = a.scale_ * b.scale_;
        emit(a, out, std::move(m));
        out.cipher_size_ = 3;
        out.scale_ = sc;
        out.relinearization_required_ = true;
        out.rescale_required_ = (S == Scheme::CKKS);
    }
    void multiply_inplace(Ciphertext<S>& a, Ciphertext<S>& b, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        multiply(a, b, a, o);
    }

    // host/ckks/operator.cuh:1053-1094: method I or II by the context's P_size
    void relinearize_inplace(Ciphertext<S>& a, Relinkey<S>& rk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!a.relinearization_required_)
            throw std::invalid_argument("Ciphertexts can not use relinearization, since no non-linear part!");
        const int l = limbs(a);
        const int op = (S == Scheme::CKKS) ? HEGPU_OP_CKKS_RELIN : HEGPU_OP_BFV_RELIN;
        detail::Workspace ws(context_->handle(), op, a.depth_, o.stream_);
        if (S == Scheme::CKKS)
            detail::check(hegpu_ckks_relinearize_inplace(context_->handle(), (uint64_t*) a.data(),
                                                         (uint64_t) 3 * l * context_->n, (const uint64_t*) rk.data(),
                                                         a.depth_, 1, ws.data(), ws.bytes, o.stream_));
        else
            detail::check(hegpu_bfv_relinearize_inplace(context_->handle(), (uint64_t*) a.data(),
                                                        (uint64_t) 3 * l * context_->n, (const uint64_t*) rk.data(), 1,
                                                        ws.data(), ws.bytes, o.stream_));
        a.relinearization_required_ = false;
        a.cipher_size_ = 2;
    }

    // host/ckks/operator.cuh:1423-1445 (CKKS only)
    void rescale_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::CKKS, "rescale is a CKKS operation");
        if (!a.rescale_required_ || a.relinearization_required_)
            throw std::invalid_argument("Ciphertexts can not be rescaled because ciphertext rescaling is not required "
                                        "or relinearization is required first!");
        const int l = limbs(a);
        if (l < 2) throw std::logic_error("Ciphertext modulus can not be reducible, since there is only one modulus");
        detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_RESCALE, a.depth_, o.stream_);
        detail::check(hegpu_ckks_rescale_inplace(context_->handle(), (uint64_t*) a.data(),
                                                 (uint64_t) 2 * l * context_->n, a.depth_, 1, ws.data(), ws.bytes,
                                                 o.stream_));
        a.scale_ = a.scale_ / (double) context_->prime_vector_[l - 1].value; // ckks/operator.cu:1235-1241
        a.depth_++;
        a.rescale_required_ = false;
    }

    // host/bfv/operator.cuh:576-660, ckks/operator.cu:1338-1378: direct key or power-of-two chain
    void rotate_rows(Ciphertext<S>& in, Ciphertext<S>& out, Galoiskey<S>& gk, int shift,
                     const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (shift == 0) { out = in; return; }
        const int g = hegpu_steps_to_galois_elt(shift, context_->n, gk.group_order_);
        if (gk.device_location_.count(g)) { apply_galois(in, out, gk, g, o); return; }
        std::vector<int> chain; // bfv/operator.cu:692-712
        int rest = std::abs(shift);
        const int sign = shift < 0 ? -1 : 1;
        while (rest) {
            const int p2 = 1 << (int) std::log2((double) rest);
            rest -= p2;
            auto it = gk.galois_elt.find(p2 * sign);
            if (it == gk.galois_elt.end() || !gk.device_location_.count(it->second))
                throw std::logic_error("Galois key not present!");
            chain.push_back(it->second);
        }
        Ciphertext<S> cur = in;
        for (int ge : chain) {
            Ciphertext<S> nxt(cur);
            apply_galois(cur, nxt, gk, ge, o);
            cur = std::move(nxt);
        }
        out = std::move(cur);
    }
    void rotate_rows_inplace(Ciphertext<S>& a, Galoiskey<S>& gk, int shift, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        Ciphertext<S> tmp(a);
        rotate_rows(tmp, a, gk, shift, o);
    }
    // Move a ciphertext to the secret key the switch key was generated for (*/operator.cuh
    // keyswitch; switchkey_*_method_I is the Galois path with the identity permutation).
    void keyswitch(Ciphertext<S>& in, Ciphertext<S>& out, Switchkey<S>& swk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!swk.switch_key_generated_) throw std::logic_error("Switchkey is not generated!");
        apply_key(in, out, (const uint64_t*) swk.data(), 1, o);
    }
    void apply_galois(Ciphertext<S>& in, Ciphertext<S>& out, Galoiskey<S>& gk, int galois_elt,
                      const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        const uint64_t* key = detail::key_for(gk, galois_elt);
        if (!key) throw std::logic_error("Galois key not present!");
        apply_key(in, out, key, galois_elt, o);
    }

    // host/ckks/operator.cuh:2133-2196 fast_single_hoisting_rotation_ckks (methods I and II by the key type):
    // result = n1 ciphertexts back to back, entry i = input rotated by bsgs_shift[i] (a zero shift: the input);
    // the INTT, the digit decomposition and the forward NTT of the digits are shared by all shifts whose
    // Galois key exists (hegpu_ckks_rotate_hoisted); a shift without its own key goes through the
    // power-of-two chain like rotate_rows (ckks/operator.cu:4833-4948), one rotation after the other.
    DeviceVector<Data64> fast_single_hoisting_rotation_ckks(Ciphertext<S>& input1, std::vector<int>& bsgs_shift, int n1,
                                                            Galoiskey<S>& galois_key, hipStream_t stream = nullptr)
    {
        static_assert(S == Scheme::CKKS, "hoisted rotations are a CKKS operation");
        ExecutionOptions o;
        o.set_stream(stream);
        detail::OpScope storage_scope(o);
        if (input1.rescale_required_ || input1.relinearization_required_)
            throw std::invalid_argument("Ciphertext can not be rotated!");
        const int l = limbs(input1);
        const size_t n = context_->n, words = 2 * n * l;
        require_words(context_, input1, 2);
        if (n1 < 1 || (size_t) n1 > bsgs_shift.size()) throw std::invalid_argument("Invalid rotation count!");
        DeviceVector<Data64> result(words * n1, stream);
        std::vector<const uint64_t*> keys(n1, nullptr);
        std::vector<int> elts(n1, 0), chained;
        for (int i = 0; i < n1; i++) {
            // the reference copies the input into entry 0 whatever bsgs_shift[0] is (method I, :4708) and treats
            // a zero shift as a copy (method II, :5138)
            if (i == 0 || bsgs_shift[i] == 0) continue;
            int g = 0;
            keys[i] = detail::key_for_shift(galois_key, bsgs_shift[i], (int) n, g);
            if (keys[i]) elts[i] = g;
            else chained.push_back(i);
        }
        detail::Workspace ws(context_->handle(), HEGPU_OP_CKKS_ROTATE_HOISTED, input1.depth_, stream);
        detail::check(hegpu_ckks_rotate_hoisted(context_->handle(), (const uint64_t*) input1.data(), 0,
                                                (uint64_t*) result.data(), 0, keys.data(), elts.data(), n1,
                                                input1.depth_, 1, ws.data(), ws.bytes, stream));
        for (int i : chained) { // no key of its own: rotate_rows' chain of power-of-two keys
            Ciphertext<S> rot(input1);
            rotate_rows(input1, rot, galois_key, bsgs_shift[i], o);
            detail::hip(hipMemcpyAsync(result.data() + (size_t) i * words, rot.data(), words * sizeof(Data64),
                                       hipMemcpyDeviceToDevice, stream));
            detail::hip(hipStreamSynchronize(stream)); // `rot` is released on return
        }
        return result;
    }

    // out = M in for the plaintext matrix of `lt` (hegpu_ckks_linear_transform: hoisted baby rotations, one pass over
    // the diagonals for all inner sums, one rotation per giant step, one sum).  The project's own addition -- the
    // reference's multiply_matrix (ckks/operator.cu:2803-2895) is private to its bootstrapping and takes pre-baked index
    // tensors.  The result is not rescaled: scale_ = in.scale_ * lt.scale(), rescale_required_ = true.  Every shift of
    // lt.required_shifts() needs a Galois key of its own: a power-of-two chain would silently multiply the key
    // switches, so a missing key is std::invalid_argument here.  A LinearTransform built with chain_giant_steps goes
    // through hegpu_ckks_linear_transform_chained with its parent table.
    void linear_transform(Ciphertext<S>& in, LinearTransform<S>& lt, Galoiskey<S>& galois_key, Ciphertext<S>& out,
                          const ExecutionOptions& o = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "linear transforms are a CKKS operation");
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (in.relinearization_required_ || in.cipher_size_ != 2)
            throw std::invalid_argument("Ciphertext should be relinearized first!");
        if (in.rescale_required_) throw std::invalid_argument("Ciphertext should be rescaled first!");
        if (in.depth_ != lt.depth()) throw std::invalid_argument("Ciphertext and LinearTransform levels are not equal");
        const int l = limbs(in);
        const size_t n = context_->n;
        require_words(context_, in, 2);
        const int n1 = lt.n1(), n2 = lt.n2();
        std::vector<const uint64_t*> keys;
        std::vector<int> elts;
        keys_of(lt, galois_key, keys, elts, "Galois key not present! (build the Galoiskey from required_shifts())");
        detail::Workspace ws(hegpu_ckks_linear_transform_workspace_bytes(context_->handle(), n1, n2, in.depth_, 1), o.stream_);
        DeviceVector<Data64> m(2 * n * l, o.stream_);
        detail::check(hegpu_ckks_linear_transform_chained(context_->handle(), (const uint64_t*) in.data(), 0,
                                                          (uint64_t*) m.data(), 0, (const uint64_t*) lt.data(),
                                                          lt.diagonal_count(), lt.index().data(), n1, n2, keys.data(),
                                                          elts.data(), keys.data() + n1, elts.data() + n1, lt.giant_parent(),
                                                          in.depth_, 1, ws.data(), ws.bytes, o.stream_));
        const double sc = in.scale_ * lt.scale();
        emit(in, out, std::move(m));
        out.scale_ = sc;
        out.rescale_required_ = true;
    }

    // The reduced Galois key set, this backend's own switch, off by default.  Read when factors are built, by
    // generate_encoding_transform_context, generate_bootstrapping_params, generate_bootstrapping_params_v2 and the logic
    // operator's generate_bootstrapping_params: the giant steps of every factor are then chained (LinearTransform's
    // chain_giant_steps), and key_indexs_ / bootstrapping_key_indexs() hold the baby steps and the links -- a subset of the
    // direct set, with the same number of key switches.
    void set_chained_giant_steps(bool on) noexcept { chained_giant_steps_ = on; }
    bool chained_giant_steps() const noexcept { return chained_giant_steps_; }

    // host/ckks/operator.cu:6686-6800.  The factors are the groups of the encoder's special FFT
    // (hegpu_encoding_transform_fill), every diagonal encoded at `scale`; the half of CoeffToSlot's real / imaginary
    // split is in its matrices.  The reference's key-chain variant (less_key_mode: its own key set, O(n2^2) key switches)
    // is not provided: std::invalid_argument; see set_chained_giant_steps above.
    void generate_encoding_transform_context(CKKSEncodingTransformContext& tc, const double scale,
                                             const CKKSEncodingTransformConfig& config = CKKSEncodingTransformConfig())
    {
        static_assert(S == Scheme::CKKS, "encoding transforms are a CKKS operation");
        if (scale == 0.0) throw std::invalid_argument("Scale can not be zero for CKKS encoding transform context.");
        if (config.CtoS_piece_ < 2 || config.CtoS_piece_ > 5) throw std::out_of_range("CtoS_piece must be in range [2, 5]");
        if (config.StoC_piece_ < 2 || config.StoC_piece_ > 5) throw std::out_of_range("StoC_piece must be in range [2, 5]");
        if (config.less_key_mode_)
            throw std::invalid_argument("less_key_mode is not supported: every rotation takes a Galois key of its own "
                                        "(the reduced key set of this backend: set_chained_giant_steps)");
        const int Q = context_->Q_size;
        const int ctos = config.CtoS_start_level_ < 0 ? 0 : config.CtoS_start_level_;
        const int stoc = config.StoC_start_level_ < 0 ? ctos + config.CtoS_piece_ + 1 : config.StoC_start_level_;
        if (ctos < 0 || ctos >= Q) throw std::out_of_range("CtoS_start_level must be in range [0, Q_size - 1]");
        if (stoc < 0 || stoc >= Q) throw std::out_of_range("StoC_start_level must be in range [0, Q_size - 1]");
        if (stoc + 1 >= Q)
            throw std::out_of_range("StoC_start_level is too deep: slot_to_coeff needs one extra level internally before "
                                    "matrix multiplication.");
        // every factor rescales and one modulus must remain (CoeffToSlot: one more level for the split), which is what
        // hegpu_ckks_coeff_to_slot / _slot_to_coeff require
        if (Q - ctos < config.CtoS_piece_ || ctos + config.CtoS_piece_ + 1 >= Q)
            throw std::out_of_range("CtoS_start_level is too deep for selected CtoS_piece.");
        if (Q - (stoc + 1) < config.StoC_piece_ || stoc + 1 + config.StoC_piece_ >= Q)
            throw std::out_of_range("StoC_start_level is too deep for selected StoC_piece.");
        tc = CKKSEncodingTransformContext();
        tc.scale_boot_ = scale;
        tc.CtoS_piece_ = config.CtoS_piece_;
        tc.StoC_piece_ = config.StoC_piece_;
        tc.less_key_mode_ = false;
        tc.CtoS_level_ = ctos;
        tc.StoC_level_ = stoc;
        // factor p at depth start + p, every one at `scale`
        const std::vector<double> scales((size_t) std::max(tc.CtoS_piece_, tc.StoC_piece_), scale);
        build_factors(1, tc.CtoS_piece_, ctos, scales.data(), tc.CtoS_factors_, tc.key_indexs_);
        build_factors(0, tc.StoC_piece_, stoc + 1, scales.data(), tc.StoC_factors_, tc.key_indexs_);
        tc.generated_ = true;
    }

    // host/ckks/operator.cu:3566-3663 (hegpu_ckks_coeff_to_slot): slot j of result 0 holds coefficient bitrev(j), of
    // result 1 coefficient N/2 + bitrev(j); both leave at CtoS_level_ + CtoS_piece_ + 1.
    std::vector<Ciphertext<S>> coeff_to_slot(Ciphertext<S>& cipher, Galoiskey<S>& galois_key,
                                             CKKSEncodingTransformContext& tc,
                                             const ExecutionOptions& o = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "encoding transforms are a CKKS operation");
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!tc.generated_) throw std::invalid_argument("Encoding transform context is not generated!");
        if (cipher.encoding_ != encoding::COEFFICIENT)
            throw std::invalid_argument("coeff_to_slot expects coefficient-encoded ciphertext.");
        if (cipher.depth_ != tc.CtoS_level_)
            throw std::logic_error("coeff_to_slot input level does not match transform_context.CtoS_start_level");
        check_plain_two_part(cipher);
        FactorArgs fa(*this, tc.CtoS_factors_, galois_key);
        const int P = tc.CtoS_piece_, out_depth = cipher.depth_ + P + 1;
        if (out_depth >= context_->Q_size) throw std::logic_error("coeff_to_slot: no modulus left for the results");
        const size_t n = context_->n, words = 2 * n * (size_t) (context_->Q_size - out_depth);
        detail::Workspace ws(hegpu_ckks_encoding_transform_workspace_bytes(context_->handle(), fa.f.data(), P, cipher.depth_, 1),
                             o.stream_);
        DeviceVector<Data64> m0(words, o.stream_), m1(words, o.stream_);
        const uint64_t* conj = conjugation_key(galois_key);
        detail::check(hegpu_ckks_coeff_to_slot(context_->handle(), (const uint64_t*) cipher.data(), 0, (uint64_t*) m0.data(),
                                               (uint64_t*) m1.data(), 0, fa.f.data(), P, conj, cipher.depth_, 1, ws.data(),
                                               ws.bytes, o.stream_));
        double sc = cipher.scale_; // every factor multiplies by its scale and the rescale divides by the modulus it drops
        for (int k = 0; k < P; k++)
            sc = sc * tc.CtoS_factors_[k]->scale() / (double) context_->prime_vector_[limbs(cipher) - 1 - k].value;
        std::vector<Ciphertext<S>> result(2, Ciphertext<S>(context_));
        for (int r = 0; r < 2; r++) {
            emit(cipher, result[r], std::move(r ? m1 : m0));
            result[r].depth_ = out_depth;
            result[r].scale_ = sc;
            result[r].encoding_ = encoding::SLOT;
        }
        return result;
    }

    // host/ckks/operator.cu:3809-3891 (hegpu_ckks_slot_to_coeff): the inverse of coeff_to_slot on inputs in its
    // bit-reversed order; the result leaves at StoC_level_ + 1 + StoC_piece_.
    Ciphertext<S> slot_to_coeff(Ciphertext<S>& cipher0, Ciphertext<S>& cipher1, Galoiskey<S>& galois_key,
                                CKKSEncodingTransformContext& tc, const ExecutionOptions& o = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "encoding transforms are a CKKS operation");
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!tc.generated_) throw std::invalid_argument("Encoding transform context is not generated!");
        if (cipher0.encoding_ != encoding::SLOT || cipher1.encoding_ != encoding::SLOT)
            throw std::invalid_argument("slot_to_coeff expects slot-encoded ciphertext inputs.");
        if (cipher0.depth_ != cipher1.depth_)
            throw std::logic_error("slot_to_coeff expects equal levels for both slot ciphertexts.");
        if (cipher0.depth_ != tc.StoC_level_)
            throw std::logic_error("slot_to_coeff input level does not match transform_context.StoC_start_level");
        check_plain_two_part(cipher0);
        check_plain_two_part(cipher1);
        FactorArgs fa(*this, tc.StoC_factors_, galois_key);
        const int P = tc.StoC_piece_, out_depth = cipher0.depth_ + 1 + P;
        if (out_depth >= context_->Q_size) throw std::logic_error("slot_to_coeff: no modulus left for the result");
        const size_t n = context_->n;
        detail::Workspace ws(hegpu_ckks_encoding_transform_workspace_bytes(context_->handle(), fa.f.data(), P, cipher0.depth_, 1),
                             o.stream_);
        DeviceVector<Data64> m(2 * n * (size_t) (context_->Q_size - out_depth + 1), o.stream_); // rescaled in place at the end
        detail::check(hegpu_ckks_slot_to_coeff(context_->handle(), (const uint64_t*) cipher0.data(), 0,
                                               (const uint64_t*) cipher1.data(), 0, (uint64_t*) m.data(), 0, fa.f.data(), P,
                                               cipher0.depth_, 1, ws.data(), ws.bytes, o.stream_));
        double sc = cipher0.scale_;
        for (int k = 0; k < P; k++)
            sc = sc * tc.StoC_factors_[k]->scale() / (double) context_->prime_vector_[limbs(cipher0) - 2 - k].value;
        Ciphertext<S> result(context_);
        emit(cipher0, result, std::move(m));
        result.depth_ = out_depth;
        result.scale_ = sc;
        result.encoding_ = encoding::COEFFICIENT;
        return result;
    }

    // pol(cipher) by the reference's baby-step/giant-step schedule (host/ckks/operator.cu:4629-4671 with gen_power,
    // evaluate_poly_recurse, evaluate_poly_from_polynomial_basis): hegpu_poly_eval_plan_* + hegpu_ckks_poly_eval.  In the
    // reference the evaluator is protected and reachable only through its bootstraps; making it public is this backend's
    // own decision (sigmoid, comparison, inverse are what a user reaches for it for).  The result carries the plan's depth
    // and scale, relinearized and rescaled.
    Ciphertext<S> evaluate_poly(Ciphertext<S>& cipher, double target_scale, const Polynomial& pol, Relinkey<S>& relin_key,
                                const ExecutionOptions& o = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "polynomial evaluation is a CKKS operation");
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        check_plain_two_part(cipher);
        if (!cipher.in_ntt_domain_) throw std::invalid_argument("Ciphertext should be in NTT domain");
        check_relin_key(relin_key);
        const int Q = context_->Q_size, level = Q - 1 - cipher.depth_;
        const std::vector<uint64_t> primes = context_primes();
        const int basis = pol.type_ == PolyType::MONOMIAL ? HEGPU_POLY_MONOMIAL : HEGPU_POLY_CHEBYSHEV;
        const double* cf = reinterpret_cast<const double*>(pol.coeffs_.data());
        const std::vector<hegpu_poly_step> plan = // too few levels: invalid_argument
            step_plan(hegpu_poly_eval_plan_size, hegpu_poly_eval_plan_fill, basis, cf, (int) pol.coeffs_.size(), pol.max_deg_,
                      pol.lead_ ? 1 : 0, level, cipher.scale_, target_scale, primes.data(), Q);
        const int n_steps = (int) plan.size();
        const hegpu_poly_step& last = plan.back();
        const size_t n = context_->n;
        detail::Workspace ws(hegpu_ckks_poly_eval_workspace_bytes(context_->handle(), plan.data(), n_steps, cipher.depth_, 1),
                             o.stream_);
        DeviceVector<Data64> m(2 * n * (size_t) (last.level + 1 + last.rescale_after), o.stream_);
        detail::check(hegpu_ckks_poly_eval(context_->handle(), (const uint64_t*) cipher.data(), 0, (uint64_t*) m.data(), 0,
                                           plan.data(), n_steps, (const uint64_t*) relin_key.data(), cipher.depth_, 1,
                                           ws.data(), ws.bytes, o.stream_));
        return evaluated(cipher, std::move(m), last.level, last.scale);
    }

    // host/ckks/operator.cu:6906-7000 (hegpu_bootstrap_plan_fill): the plan of the refresh for ciphertexts
    // of `scale`, its EvalMod plan and the factors of both transforms, every diagonal encoded at the level and scale the
    // plan gives it.  A transform of P pieces spends P + 1 levels here (its factors and the limb the boundary pass drops;
    // the reference: P), so CoeffToSlot takes cts_config_.level_start_ - eval_mod_config_.level_start_ - 1 pieces
    // whatever cts_config_.piece_ says, SlotToCoeff takes stc_config_.piece_ and the result leaves at
    // stc_config_.level_start_ - 1 - piece_, one level below the reference's.  Locked after the first call.
    void generate_bootstrapping_params_v2(const double scale, const BootstrappingConfigV2& config)
    {
        static_assert(S == Scheme::CKKS, "bootstrapping parameters are a CKKS matter");
        if (boot_v2_.generated || slim_.generated)
            throw std::runtime_error("Bootstrapping parameters is locked after generation and cannot be modified.");
        detail::require_generated(context_);
        const EvalModConfig& em = config.eval_mod_config_;
        if (em.sine_type_ != SineType::COS1) throw std::invalid_argument("Unsupported sine type!");
        if (em.arcsine_deg_ != 0) throw std::invalid_argument("The arcsine correction is not supported!");
        const int Q = context_->Q_size;
        const std::vector<uint64_t> primes = context_primes();
        hegpu_bootstrap_config cfg{};
        cfg.scale = scale;
        cfg.message_ratio = em.message_ratio_;
        cfg.K = em.K_;
        cfg.sine_degree = em.sine_deg_;
        cfg.double_angle = em.double_angle_;
        cfg.cts_level = config.cts_config_.level_start_;
        cfg.cts_pieces = config.cts_config_.level_start_ - em.level_start_ - 1;
        cfg.eval_level = em.level_start_;
        cfg.stc_level = config.stc_config_.level_start_;
        cfg.stc_pieces = config.stc_config_.piece_;
        BootV2 b;
        detail::check(hegpu_bootstrap_plan_fill(&cfg, primes.data(), Q, &b.plan));
        b.eval_mod = step_plan(hegpu_eval_mod_plan_size, hegpu_eval_mod_plan_fill, b.plan.K, b.plan.sine_degree, b.plan.double_angle,
                               b.plan.eval_level, b.plan.eval_in_scale, b.plan.eval_target_scale, primes.data(), Q);
        // factor p at depth Q - 1 - (first_level - p), first_level = cts_level resp. stc_level - 1
        build_factors(1, b.plan.cts_pieces, Q - 1 - b.plan.cts_level, b.plan.cts_scale, b.cts, b.key_indexs);
        build_factors(0, b.plan.stc_pieces, Q - 1 - (b.plan.stc_level - 1), b.plan.stc_scale, b.stc, b.key_indexs);
        b.scale = scale;
        b.generated = true;
        boot_v2_ = std::move(b);
    }
    // every rotation of every factor: Galoiskey(context, bootstrapping_key_indexs()) is enough (the conjugation is in
    // every Galoiskey); serves both parameter sets, of which one is generated
    std::vector<int> bootstrapping_key_indexs() const { return slim_.generated ? slim_.key_indexs : boot_v2_.key_indexs; }

    // host/ckks/operator.cu:7147-7224 (hegpu_ckks_bootstrap): the refresh of a ciphertext at its last level.  The two switch
    // keys of mod_up_from_q0 (to an ephemeral sparse secret before the raise and back after it) are both given or both
    // null.  The result carries the scale the parameters were generated for, at the plan's level; its coefficients are
    // (rho / 2 pi) sin(2 pi a / rho) of the input's, rho = q_0 / (k1 scale).
    Ciphertext<S> regular_bootstrapping_v2(Ciphertext<S>& input1, Galoiskey<S>& galois_key, Relinkey<S>& relin_key,
                                           Switchkey<S>* swk_dense_to_sparse = nullptr,
                                           Switchkey<S>* swk_sparse_to_dense = nullptr,
                                           const ExecutionOptions& options = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "regular bootstrapping is a CKKS operation");
        if (!boot_v2_.generated)
            throw std::invalid_argument("Bootstrapping operation can not be performed before generating Bootstrapping parameters!");
        if (context_->Q_size - input1.depth_ != 1) throw std::logic_error("Ciphertexts leveled should be at max!");
        detail::OpScope storage_scope(options); // storage manager: stage HOST-stored operands, place the results
        check_plain_two_part(input1);
        if (!input1.in_ntt_domain_) throw std::invalid_argument("Ciphertext should be in NTT domain");
        check_relin_key(relin_key);
        if (!swk_dense_to_sparse != !swk_sparse_to_dense)
            throw std::invalid_argument("Both switch keys (dense to sparse, sparse to dense) or neither!");
        for (Switchkey<S>* k : {swk_dense_to_sparse, swk_sparse_to_dense})
            if (k && !k->switch_key_generated_) throw std::logic_error("Switchkey is not generated!");
        FactorArgs fc(*this, boot_v2_.cts, galois_key), fs(*this, boot_v2_.stc, galois_key);
        const uint64_t* conj = conjugation_key(galois_key);
        const hegpu_bootstrap_plan& p = boot_v2_.plan;
        const int n_steps = (int) boot_v2_.eval_mod.size();
        const uint64_t* down = swk_dense_to_sparse ? (const uint64_t*) swk_dense_to_sparse->data() : nullptr;
        const uint64_t* up = swk_sparse_to_dense ? (const uint64_t*) swk_sparse_to_dense->data() : nullptr;
        detail::Workspace ws(hegpu_ckks_bootstrap_workspace_bytes(context_->handle(), &p, boot_v2_.eval_mod.data(), n_steps,
                                                                  fc.f.data(), p.cts_pieces, fs.f.data(), p.stc_pieces,
                                                                  down ? 1 : 0, 1),
                             options.stream_);
        DeviceVector<Data64> m(2 * context_->n * (size_t) (p.out_level + 2), options.stream_); // rescaled in place at the end
        detail::check(hegpu_ckks_bootstrap(context_->handle(), (const uint64_t*) input1.data(), 0, (uint64_t*) m.data(), 0, &p,
                                           boot_v2_.eval_mod.data(), n_steps, fc.f.data(), p.cts_pieces, fs.f.data(),
                                           p.stc_pieces, conj, (const uint64_t*) relin_key.data(), down, up, 1, ws.data(),
                                           ws.bytes, options.stream_));
        return evaluated(input1, std::move(m), p.out_level, p.out_scale);
    }

    // ---- the slim family (host/ckks/operator.cu:6800-6900, :7226-7330): SlotToCoeff first at the bottom
    // of the chain, the raise, CoeffToSlot, the real parts, ONE polynomial alpha + A cos(2 pi (K u - phi)).
    // Departures from the reference, which builds this family on its Taylor exp_scaled and v1 Vandermonde machinery:
    //  * taylor_number_ and less_key_mode_ are carried and unused: the polynomial is the Chebyshev cosine with K = 12,
    //    degree 30 and three double angles, the plan of hegpu_slim_bootstrap_plan_fill;
    //  * the result's scale_ is the plan's out_scale (for slim: q_(eval level) / 256 to the rounding of doubles), not the
    //    scale the parameters were generated for; its slots are (rho / 2 pi) sin(2 pi z / rho), rho = 256;
    //  * CoeffToSlot spends CtoS_piece_ + 1 levels (its factors and the limb the real part drops), as in 4.5f;
    //  * REGULAR_BOOTSTRAPPING through this call is not built (std::invalid_argument): the regular refresh is
    //    generate_bootstrapping_params_v2 / regular_bootstrapping_v2.
    // Locked after the first call, together with generate_bootstrapping_params_v2, as the reference's one flag does.
    void generate_bootstrapping_params(const double scale, const BootstrappingConfig& config,
                                       const arithmetic_bootstrapping_type& boot_type)
    {
        static_assert(S == Scheme::CKKS, "bootstrapping parameters are a CKKS matter");
        if (boot_type == arithmetic_bootstrapping_type::REGULAR_BOOTSTRAPPING)
            throw std::invalid_argument("REGULAR_BOOTSTRAPPING is not built on this parameter set: use "
                                        "generate_bootstrapping_params_v2 and regular_bootstrapping_v2!");
        if (boot_type != arithmetic_bootstrapping_type::SLIM_BOOTSTRAPPING) throw std::invalid_argument("Invalid Bootstrapping Type");
        generate_slim_family_params(scale, config, 256.0, true);
    }
    Ciphertext<S> slim_bootstrapping(Ciphertext<S>& input1, Galoiskey<S>& galois_key, Relinkey<S>& relin_key,
                                     const ExecutionOptions& options = ExecutionOptions())
    {
        return slim_family_bootstrapping(SLIM_FUNCTION, input1, nullptr, galois_key, relin_key, options);
    }
    // This backend's seam under slim_bootstrapping and HELogicOperator<CKKS>'s bit and gate bootstrapping: one parameter
    // set per ratio q_0 / (scale of the raised coefficients) -- 256 slim, 2 bit, 3 gates -- and one plan per function.
    enum { SLIM_FUNCTION = 0, BIT_FUNCTION, AND_FUNCTION, OR_FUNCTION, XOR_FUNCTION, NAND_FUNCTION, NOR_FUNCTION, XNOR_FUNCTION,
           SLIM_FAMILY_SIZE };
    void generate_slim_family_params(const double scale, const BootstrappingConfig& config, double ratio, bool arithmetic)
    {
        static_assert(S == Scheme::CKKS, "bootstrapping parameters are a CKKS matter");
        if (boot_v2_.generated || slim_.generated)
            throw std::runtime_error("Bootstrapping parameters is locked after generation and cannot be modified.");
        detail::require_generated(context_);
        const int Q = context_->Q_size;
        const std::vector<uint64_t> primes = context_primes();
        // (phi, A, alpha) of alpha + A cos(2 pi (a / ratio - phi)), include/hegpu.h
        static const double family[SLIM_FAMILY_SIZE][3] = {
            {0.25, 1.0 / (2.0 * 3.14159265358979323846), 0.0}, {1.0 / 2, 1.0 / 2, 1.0 / 2},
            {2.0 / 3, 2.0 / 3, 1.0 / 3}, {1.0 / 2, 2.0 / 3, 2.0 / 3}, {1.0 / 3, 2.0 / 3, 1.0 / 3},
            {1.0 / 6, 2.0 / 3, 2.0 / 3}, {0.0, 2.0 / 3, 1.0 / 3},     {5.0 / 6, 2.0 / 3, 2.0 / 3}};
        SlimBoot b;
        for (int fn = 0; fn < SLIM_FAMILY_SIZE; fn++) {
            const bool wanted = arithmetic ? fn == SLIM_FUNCTION : ratio == 2.0 ? fn == BIT_FUNCTION : fn >= AND_FUNCTION;
            if (!wanted) continue;
            hegpu_slim_bootstrap_config cfg{};
            cfg.scale = scale;
            cfg.ratio = ratio;
            cfg.phase = family[fn][0];
            cfg.amplitude = family[fn][1];
            cfg.offset = family[fn][2];
            cfg.K = 12;
            cfg.degree = 30;
            cfg.double_angle = 3;
            cfg.cts_level = Q - 1;
            cfg.cts_pieces = config.CtoS_piece_;
            cfg.stc_pieces = config.StoC_piece_;
            cfg.arithmetic = arithmetic ? 1 : 0;
            hegpu_slim_bootstrap_plan& p = b.plan[fn];
            detail::check(hegpu_slim_bootstrap_plan_fill(&cfg, primes.data(), Q, &p));
            b.trig[fn] = step_plan(hegpu_eval_trig_plan_size, hegpu_eval_trig_plan_fill, p.K, p.degree, p.double_angle, p.phase,
                                   p.amplitude, p.offset, p.eval_level, p.eval_in_scale, p.eval_target_scale, primes.data(), Q);
            b.first = b.first < 0 ? fn : b.first;
        }
        // the factors depend on the function through its ratio alone: one set serves every plan of the set
        const hegpu_slim_bootstrap_plan& p0 = b.plan[b.first];
        // factor p at depth Q - 1 - (first_level - p), first_level = cts_level resp. in_level
        build_factors(1, p0.cts_pieces, Q - 1 - p0.cts_level, p0.cts_scale, b.cts, b.key_indexs);
        build_factors(0, p0.stc_pieces, Q - 1 - p0.in_level, p0.stc_scale, b.stc, b.key_indexs);
        b.generated = true;
        slim_ = std::move(b);
    }
    bool slim_family_generated() const { return slim_.generated; }
    // input1 (and input2 for a gate) at level StoC_piece_: the reference's "Ciphertexts leveled should be at max!"
    Ciphertext<S> slim_family_bootstrapping(int function, Ciphertext<S>& input1, Ciphertext<S>* input2, Galoiskey<S>& galois_key,
                                            Relinkey<S>& relin_key, const ExecutionOptions& options = ExecutionOptions())
    {
        static_assert(S == Scheme::CKKS, "bootstrapping is a CKKS operation");
        if (!slim_.generated || function < 0 || function >= SLIM_FAMILY_SIZE || slim_.trig[function].empty())
            throw std::invalid_argument("Bootstrapping operation can not be performed before generating Bootstrapping parameters!");
        const hegpu_slim_bootstrap_plan& p = slim_.plan[function];
        for (Ciphertext<S>* in : {&input1, input2})
            if (in && context_->Q_size - in->depth_ != 1 + p.stc_pieces) throw std::logic_error("Ciphertexts leveled should be at max!");
        detail::OpScope storage_scope(options); // storage manager: stage HOST-stored operands, place the results
        for (Ciphertext<S>* in : {&input1, input2}) {
            if (!in) continue;
            check_plain_two_part(*in);
            if (!in->in_ntt_domain_) throw std::invalid_argument("Ciphertext should be in NTT domain");
        }
        check_relin_key(relin_key);
        FactorArgs fc(*this, slim_.cts, galois_key), fs(*this, slim_.stc, galois_key);
        const uint64_t* conj = conjugation_key(galois_key);
        const std::vector<hegpu_poly_step>& trig = slim_.trig[function];
        const int n_steps = (int) trig.size();
        const hegpu_poly_step& last = trig.back();
        detail::Workspace ws(hegpu_ckks_slim_bootstrap_workspace_bytes(context_->handle(), &p, trig.data(), n_steps, fc.f.data(),
                                                                       p.cts_pieces, fs.f.data(), p.stc_pieces, 1),
                             options.stream_);
        DeviceVector<Data64> m(2 * context_->n * (size_t) (p.out_level + 1 + (last.rescale_after ? 1 : 0)), options.stream_);
        detail::check(hegpu_ckks_slim_bootstrap(context_->handle(), (const uint64_t*) input1.data(), 0,
                                                input2 ? (const uint64_t*) input2->data() : nullptr, 0, (uint64_t*) m.data(), 0,
                                                &p, trig.data(), n_steps, fc.f.data(), p.cts_pieces, fs.f.data(), p.stc_pieces,
                                                conj, (const uint64_t*) relin_key.data(), 1, ws.data(), ws.bytes,
                                                options.stream_));
        return evaluated(input1, std::move(m), p.out_level, p.out_scale);
    }

  private:
    // the factors of both transforms and every shift they rotate by
    struct RefreshFactors {
        std::vector<std::shared_ptr<LinearTransform<S>>> cts, stc;
        std::vector<int> key_indexs;
    };
    // what generate_slim_family_params leaves for slim_family_bootstrapping: a plan per function of the set, one set of factors
    struct SlimBoot : RefreshFactors {
        bool generated = false;
        int first = -1;
        hegpu_slim_bootstrap_plan plan[SLIM_FAMILY_SIZE]{};
        std::vector<hegpu_poly_step> trig[SLIM_FAMILY_SIZE];
    };
    SlimBoot slim_;
    // what generate_bootstrapping_params_v2 leaves for regular_bootstrapping_v2
    struct BootV2 : RefreshFactors {
        bool generated = false;
        double scale = 0.0;
        hegpu_bootstrap_plan plan{};
        std::vector<hegpu_poly_step> eval_mod;
    };
    BootV2 boot_v2_;
    bool chained_giant_steps_ = false; // set_chained_giant_steps
    // One chain of factors of the encoder's special FFT (hegpu_encoding_transform_shape / _fill; inverse: CoeffToSlot) in the
    // order they are applied: factor p, its diagonals encoded at scales[p] and depth `depth` + p, is appended to `factors`,
    // the shifts it rotates by to `key_indexs`.  With set_chained_giant_steps(true) the factors' giant steps are chained.
    void build_factors(int inverse, int pieces, int depth, const double* scales,
                       std::vector<std::shared_ptr<LinearTransform<S>>>& factors, std::vector<int>& key_indexs)
    {
        HEEncoder<S> encoder(context_);
        const int n = (int) context_->n, slots = n >> 1;
        std::vector<int> strides(pieces), stages(pieces), counts(pieces);
        detail::check(hegpu_encoding_transform_shape(n, inverse, pieces, strides.data(), stages.data(), counts.data()));
        for (int p = 0; p < pieces; p++) {
            std::vector<int> offsets(counts[p]);
            std::vector<double> values((size_t) 2 * counts[p] * slots);
            detail::check(hegpu_encoding_transform_fill(n, inverse, pieces, p, counts[p], offsets.data(), values.data()));
            std::map<int, std::vector<Complex64>> diag;
            for (int d = 0; d < counts[p]; d++) {
                std::vector<Complex64> v((size_t) slots);
                for (int t = 0; t < slots; t++)
                    v[t] = Complex64(values[2 * ((size_t) d * slots + t)], values[2 * ((size_t) d * slots + t) + 1]);
                diag[offsets[d]] = std::move(v);
            }
            auto lt = std::make_shared<LinearTransform<S>>(context_, diag, encoder, scales[p], depth + p, 0, ExecutionOptions(),
                                                           strides[p], chained_giant_steps_);
            for (int sh : lt->required_shifts())
                if (std::find(key_indexs.begin(), key_indexs.end(), sh) == key_indexs.end()) key_indexs.push_back(sh);
            factors.push_back(std::move(lt));
        }
    }
    std::vector<uint64_t> context_primes() const
    {
        std::vector<uint64_t> primes((size_t) context_->Q_size);
        for (size_t i = 0; i < primes.size(); i++) primes[i] = context_->prime_vector_[i].value;
        return primes;
    }
    // a step plan of the C ABI: size(args..., &n_steps), then fill(args..., steps, n_steps)
    template <typename Size, typename Fill, typename... Args>
    static std::vector<hegpu_poly_step> step_plan(Size size, Fill fill, Args... args)
    {
        int n_steps = 0;
        detail::check(size(args..., &n_steps));
        std::vector<hegpu_poly_step> plan((size_t) n_steps);
        detail::check(fill(args..., plan.data(), n_steps));
        return plan;
    }
    void check_relin_key(Relinkey<S>& relin_key) const
    {
        if (!relin_key.relin_key_generated_ || relin_key.size() != detail::KeySwitchShape(context_).size())
            throw std::invalid_argument("Relinkey does not belong to this context!");
    }
    const uint64_t* conjugation_key(Galoiskey<S>& galois_key) const
    {
        const uint64_t* conj = detail::key_for(galois_key, galois_key.galois_elt_zero);
        if (!conj) throw std::invalid_argument("Galois key not present! (conjugation)");
        return conj;
    }
    // the result of a step plan or a refresh: `m` with in's other properties, relinearized and rescaled
    Ciphertext<S> evaluated(const Ciphertext<S>& in, DeviceVector<Data64>&& m, int level, double scale) const
    {
        Ciphertext<S> result(context_);
        emit(in, result, std::move(m));
        result.depth_ = context_->Q_size - 1 - level;
        result.scale_ = scale;
        result.rescale_required_ = false;
        result.relinearization_required_ = false;
        return result;
    }
    void check_plain_two_part(const Ciphertext<S>& a) const
    {
        if (a.relinearization_required_ || a.cipher_size_ != 2)
            throw std::invalid_argument("Ciphertext should be relinearized first!");
        if (a.rescale_required_) throw std::invalid_argument("Ciphertext should be rescaled first!");
        require_words(context_, a, 2);
    }
    // the keys and Galois elements of a LinearTransform's baby steps, then its giant steps or their links (a zero shift takes none); a
    // power-of-two chain would silently multiply the key switches, so a missing key is std::invalid_argument(`hint`)
    void keys_of(const LinearTransform<S>& lt, Galoiskey<S>& gk, std::vector<const uint64_t*>& keys, std::vector<int>& elts,
                 const char* hint) const
    {
        const int n1 = lt.n1(), n2 = lt.n2();
        keys.assign(n1 + n2, nullptr);
        elts.assign(n1 + n2, 0);
        for (int i = 0; i < n1 + n2; i++) {
            const int shift = i < n1 ? lt.baby_shifts()[i] : lt.link_shifts()[i - n1];
            if (shift == 0) continue;
            keys[i] = detail::key_for_shift(gk, shift, (int) context_->n, elts[i]);
            if (!keys[i]) throw std::invalid_argument(hint);
        }
    }
    // the hegpu_linear_factor array of a chain of LinearTransform objects, with the key and element tables it points into
    struct FactorArgs {
        std::vector<std::vector<const uint64_t*>> keys;
        std::vector<std::vector<int>> elts;
        std::vector<hegpu_linear_factor> f;
        FactorArgs(HEArithmeticOperator& op, const std::vector<std::shared_ptr<LinearTransform<S>>>& lts, Galoiskey<S>& gk)
            : keys(lts.size()), elts(lts.size()), f(lts.size())
        {
            for (size_t k = 0; k < lts.size(); k++) {
                const LinearTransform<S>& lt = *lts[k];
                const int n1 = lt.n1(), n2 = lt.n2();
                op.keys_of(lt, gk, keys[k], elts[k], "Galois key not present! (build the Galoiskey from key_indexs_)");
                f[k] = hegpu_linear_factor{(const uint64_t*) lt.data(), lt.diagonal_count(), lt.index().data(), n1, n2,
                                           keys[k].data(), elts[k].data(), keys[k].data() + n1, elts[k].data() + n1,
                                           lt.giant_parent()};
            }
        }
    };
    void apply_key(Ciphertext<S>& in, Ciphertext<S>& out, const uint64_t* key, int galois_elt, const ExecutionOptions& o)
    {
        if (in.relinearization_required_) throw std::invalid_argument("Ciphertext should be relinearized first!");
        const int l = limbs(in);
        const size_t n = context_->n;
        DeviceVector<Data64> m(2 * n * l, o.stream_);
        const int op = (S == Scheme::CKKS) ? HEGPU_OP_CKKS_GALOIS : HEGPU_OP_BFV_GALOIS;
        detail::Workspace ws(context_->handle(), op, in.depth_, o.stream_);
        if (S == Scheme::CKKS)
            detail::check(hegpu_ckks_apply_galois(context_->handle(), (const uint64_t*) in.data(), 0, (uint64_t*) m.data(), 0,
                                                  key, galois_elt, in.depth_, 1, ws.data(), ws.bytes, o.stream_));
        else
            detail::check(hegpu_bfv_apply_galois(context_->handle(), (const uint64_t*) in.data(), 0, (uint64_t*) m.data(), 0,
                                                 key, galois_elt, 1, ws.data(), ws.bytes, o.stream_));
        emit(in, out, std::move(m));
    }

  public:
    // the in-place forms go through the out-of-place operators, so each of them runs inside a storage scope
    void add_inplace(Ciphertext<S>& a, Ciphertext<S>& b, const ExecutionOptions& o = ExecutionOptions()) { add(a, b, a, o); }
    void sub_inplace(Ciphertext<S>& a, Ciphertext<S>& b, const ExecutionOptions& o = ExecutionOptions()) { sub(a, b, a, o); }
    void negate_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions()) { negate(a, a, o); }
    // CKKS: drop the last limb without dividing (ckks/operator.cuh mod_drop*)
    void mod_drop(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::CKKS, "mod_drop is a CKKS operation");
        const int l = limbs(a);
        if (l < 2) throw std::logic_error("Ciphertext modulus can not be reducible, since there is only one modulus");
        const size_t n = context_->n;
        DeviceVector<Data64> m((size_t) a.cipher_size_ * (l - 1) * n, o.stream_);
        for (int p = 0; p < a.cipher_size_; p++)
            detail::hip(hipMemcpyAsync(m.data() + (size_t) p * (l - 1) * n, a.data() + (size_t) p * l * n,
                                       (size_t) (l - 1) * n * sizeof(Data64), hipMemcpyDeviceToDevice, o.stream_));
        const int depth = a.depth_ + 1;
        emit(a, out, std::move(m));
        out.depth_ = depth;
    }
    void mod_drop_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions()) { mod_drop(a, a, o); }
    void mod_drop_inplace(Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::CKKS, "mod_drop is a CKKS operation");
        const int l = context_->Q_size - p.depth_;
        if (l < 2) throw std::logic_error("Plaintext modulus can not be reducible, since there is only one modulus");
        DeviceVector<Data64> m((size_t) (l - 1) * context_->n, o.stream_);
        detail::hip(hipMemcpyAsync(m.data(), p.data(), m.size() * sizeof(Data64), hipMemcpyDeviceToDevice, o.stream_));
        p.memory_set(std::move(m));
        p.depth_++;
    }

    // ---- ciphertext (+,-,*) plaintext (host/*/operator.cuh add_plain / sub_plain / multiply_plain)
    void add_plain(Ciphertext<S>& a, Plaintext<S>& p, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        plain_addsub(a, p, out, 0, o);
    }
    void sub_plain(Ciphertext<S>& a, Plaintext<S>& p, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        plain_addsub(a, p, out, 1, o);
    }
    void add_plain_inplace(Ciphertext<S>& a, Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        plain_addsub(a, p, a, 0, o);
    }
    void sub_plain_inplace(Ciphertext<S>& a, Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        plain_addsub(a, p, a, 1, o);
    }
    void multiply_plain(Ciphertext<S>& a, Plaintext<S>& p, Ciphertext<S>& out,
                        const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (a.relinearization_required_) throw std::invalid_argument("Ciphertext should be relinearized first!");
        const int l = limbs(a);
        const size_t n = context_->n;
        DeviceVector<Data64> m(2 * n * l, o.stream_);
        if (S == Scheme::CKKS) {
            if (a.rescale_required_) throw std::invalid_argument("Ciphertext should be rescaled first!");
            if (p.depth_ != a.depth_) throw std::logic_error("Ciphertext and Plaintext levels are not equal");
            detail::check(hegpu_cipherplain_multiplication(context_->handle(), (const uint64_t*) a.data(),
                                                           (const uint64_t*) p.data(), (uint64_t*) m.data(), l,
                                                           o.stream_));
        } else if (a.in_ntt_domain_ != p.in_ntt_domain_) {
            throw std::logic_error("BFV ciphertext or plaintext should be not in same domain"); // bfv/operator.cuh:447
        } else if (a.in_ntt_domain_) { // both transformed: one pointwise product (bfv/operator.cu:441-449)
            detail::check(hegpu_cipherplain_multiplication(context_->handle(), (const uint64_t*) a.data(),
                                                           (const uint64_t*) p.data(), (uint64_t*) m.data(), l,
                                                           o.stream_));
        } else {
            detail::Workspace ws(context_->handle(), HEGPU_OP_BFV_MULTIPLY_PLAIN, 0, o.stream_);
            detail::check(hegpu_bfv_multiply_plain(context_->handle(), (const uint64_t*) a.data(),
                                                   (const uint64_t*) p.data(), (uint64_t*) m.data(), ws.data(), ws.bytes,
                                                   o.stream_));
        }
        const double ps = p.scale_;
        emit(a, out, std::move(m));
        if (S == Scheme::CKKS) {
            out.scale_ = a.scale_ * ps; // ckks/operator.cuh multiply_plain
            out.rescale_required_ = true;
        }
    }
    void multiply_plain_inplace(Ciphertext<S>& a, Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        multiply_plain(a, p, a, o);
    }

    // ---- BFV: domain changes and X^k (bfv/operator.cuh:884-1110)
    void transform_to_ntt(Plaintext<S>& p, Plaintext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::BFV, "BFV operation");
        if (p.in_ntt_domain_) { if (&p != &out) out = p; return; }
        if (p.size() < (size_t) context_->n) throw std::invalid_argument("Invalid Ciphertexts size!");
        DeviceVector<Data64> m((size_t) context_->Q_size * context_->n, o.stream_);
        detail::check(hegpu_bfv_plain_to_ntt(context_->handle(), (const uint64_t*) p.data(), (uint64_t*) m.data(), o.stream_));
        if (&p != &out) out = p;
        out.memory_set(std::move(m));
        out.in_ntt_domain_ = true;
    }
    void transform_to_ntt_inplace(Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions()) { transform_to_ntt(p, p, o); }
    void transform_to_ntt(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::BFV, "BFV operation");
        if (a.relinearization_required_) throw std::invalid_argument("Ciphertexts can not be transformed to NTT!");
        change_domain(a, out, false, o);
    }
    void transform_to_ntt_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions()) { transform_to_ntt(a, a, o); }
    void transform_from_ntt(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::BFV, "BFV operation");
        if (a.relinearization_required_) throw std::invalid_argument("Ciphertexts can not be transformed from NTT!");
        change_domain(a, out, true, o);
    }
    void transform_from_ntt_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions()) { transform_from_ntt(a, a, o); }
    void multiply_power_of_X(Ciphertext<S>& a, Ciphertext<S>& out, int index, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::BFV, "BFV operation");
        if (index == 0) return; // the reference leaves `out` untouched (bfv/operator.cuh:889)
        if (a.in_ntt_domain_) throw std::invalid_argument("Ciphertext should be in intt domain");
        if (a.memory_size() < (size_t) 2 * context_->n * context_->Q_size) throw std::invalid_argument("Invalid Ciphertexts size!");
        DeviceVector<Data64> m((size_t) 2 * context_->Q_size * context_->n, o.stream_);
        detail::check(hegpu_negacyclic_shift(context_->handle(), (const uint64_t*) a.data(), (uint64_t*) m.data(), index,
                                             context_->Q_size, 2, o.stream_));
        emit(a, out, std::move(m));
    }

    // ---- CKKS: one real constant in every slot (ckks/operator.cuh:312-390, :507-585, :812-925), +-i, conjugation
    void add_plain(Ciphertext<S>& a, double c, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (a.relinearization_required_)
            throw std::invalid_argument("Ciphertext and Plaintext can not be added because ciphertext has non-linear partl!");
        constant_op(HEGPU_CONST_ADD, a, c * a.scale_, out, o);
    }
    void add_plain_inplace(Ciphertext<S>& a, double c, const ExecutionOptions& o = ExecutionOptions()) { add_plain(a, c, a, o); }
    void sub_plain(Ciphertext<S>& a, double c, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (a.relinearization_required_)
            throw std::invalid_argument("Ciphertext and Plaintext can not be added because ciphertext has non-linear partl!");
        constant_op(HEGPU_CONST_SUB, a, c * a.scale_, out, o);
    }
    void sub_plain_inplace(Ciphertext<S>& a, double c, const ExecutionOptions& o = ExecutionOptions()) { sub_plain(a, c, a, o); }
    void multiply_plain(Ciphertext<S>& a, double c, Ciphertext<S>& out, double scale,
                        const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (a.relinearization_required_)
            throw std::invalid_argument("Ciphertext and Plaintext can not be multiplied because of the non-linear part! "
                                        "Please use relinearization operation!");
        const double in_scale = a.scale_;
        constant_op(HEGPU_CONST_MUL, a, c * scale, out, o);
        out.scale_ = in_scale * scale; // multiply_const_plain_ckks, operator.cu:893
        out.rescale_required_ = true;
    }
    void multiply_plain_inplace(Ciphertext<S>& a, double c, double scale, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        multiply_plain(a, c, a, scale, o);
    }
    // host/ckks/operator.cuh:586-926: a complex constant in every slot (add_constant_plain_ckks_v2 /
    // multiply_const_plain_ckks_v2, ckks/operator.cu:567-724) and scale_up (:726-740)
    void add_plain_v2(Ciphertext<S>& a, Complex64 c, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o);
        gaussian(a, out, 0, c.real() * a.scale_, c.imag() * a.scale_, o);
    }
    void multiply_plain_v2(Ciphertext<S>& a, Complex64 c, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o);
        // a constant with a fractional part is scaled by the current last modulus (ckks/operator.cu:648-677)
        auto fractional = [](double v) { return v != 0 && (v - (double) (std::int64_t) v) != 0; };
        double factor = 1.0;
        if (fractional(c.real()) || fractional(c.imag())) factor = (double) context_->prime_vector_[limbs(a) - 1].value;
        const double sc = a.scale_ * factor;
        gaussian(a, out, 1, c.real() * factor, c.imag() * factor, o);
        out.scale_ = sc;
    }
    void scale_up(Ciphertext<S>& a, double scale, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o);
        const double sc = a.scale_ * scale; // the original scale, not its integer part (:737-739)
        gaussian(a, out, 1, (double) (std::uint64_t) scale, 0.0, o);
        out.scale_ = sc;
    }
    void mult_i(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions()) { times_i(a, out, 0, o); }
    void div_i(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions()) { times_i(a, out, 1, o); }
    // complex conjugate of every slot: the Galois element 2N - 1 (conjugate_ckks_method_I/II)
    void conjugate(Ciphertext<S>& in, Ciphertext<S>& out, Galoiskey<S>& gk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        static_assert(S == Scheme::CKKS, "conjugate is a CKKS operation");
        apply_galois(in, out, gk, gk.galois_elt_zero, o);
    }
    void apply_galois_inplace(Ciphertext<S>& a, Galoiskey<S>& gk, int galois_elt, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        Ciphertext<S> tmp(a);
        apply_galois(tmp, a, gk, galois_elt, o);
    }
    void mod_drop(Plaintext<S>& p, Plaintext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        out = p;
        mod_drop_inplace(out, o);
    }
    // BFV: swap the two rows of the slot matrix (Galois element 2N - 1, bfv/operator.cu:975-1068)
    void rotate_columns(Ciphertext<S>& in, Ciphertext<S>& out, Galoiskey<S>& gk,
                        const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        apply_galois(in, out, gk, gk.galois_elt_zero, o);
    }

  private:
    int limbs(const Ciphertext<S>& a) const { return context_->Q_size - a.depth_; }
    static void copy_meta(const Ciphertext<S>& a, Ciphertext<S>& out)
    {
        out.ring_size_ = a.ring_size_;
        out.coeff_modulus_count_ = a.coeff_modulus_count_;
        out.cipher_size_ = a.cipher_size_;
        out.depth_ = a.depth_;
        out.scale_ = a.scale_;
        out.in_ntt_domain_ = a.in_ntt_domain_;
        out.rescale_required_ = a.rescale_required_;
        out.relinearization_required_ = a.relinearization_required_;
    }
    // the tail of an operator: `out` describes itself like `in` and owns the fresh residues; what the operator changes
    // (depth, scale, flags) it sets afterwards
    static void emit(const Ciphertext<S>& in, Ciphertext<S>& out, DeviceVector<Data64>&& m)
    {
        if (&in != &out) copy_meta(in, out);
        out.memory_set(std::move(m));
        out.ciphertext_generated_ = true;
    }
    // `parts` polynomials at the ciphertext's own level have to be there before a kernel reads them
    static void require_words(const HEContext<S>& c, const Ciphertext<S>& ct, int parts)
    {
        if (ct.memory_size() < (size_t) parts * (c->Q_size - ct.depth_) * c->n) throw std::invalid_argument("Invalid Ciphertexts size!");
    }
    void binary(Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& out, int op, const ExecutionOptions& o)
    {
        if (a.depth_ != b.depth_) throw std::logic_error("Ciphertexts leveled are not equal");
        if (a.cipher_size_ != b.cipher_size_) throw std::invalid_argument("Ciphertexts sizes have to be equal");
        const int l = limbs(a);
        DeviceVector<Data64> m((size_t) a.cipher_size_ * l * context_->n, o.stream_);
        detail::check(hegpu_addition(context_->handle(), (const uint64_t*) a.data(), (const uint64_t*) b.data(),
                                     (uint64_t*) m.data(), l, a.cipher_size_, 1, op, o.stream_));
        emit(a, out, std::move(m));
    }
    void change_domain(Ciphertext<S>& a, Ciphertext<S>& out, bool inverse, const ExecutionOptions& o)
    {
        if (a.in_ntt_domain_ == !inverse) { if (&a != &out) out = a; return; } // already there
        const int Q = context_->Q_size;
        if (a.memory_size() < (size_t) 2 * context_->n * Q) throw std::invalid_argument("Invalid Ciphertexts size!");
        DeviceVector<Data64> m((size_t) 2 * Q * context_->n, o.stream_);
        detail::check(hegpu_ntt(context_->handle(), HEGPU_TABLES_QP, (const uint64_t*) a.data(), (uint64_t*) m.data(),
                                inverse ? 1 : 0, 2 * Q, Q, 0, nullptr, nullptr, o.stream_));
        emit(a, out, std::move(m));
        out.in_ntt_domain_ = !inverse;
    }
    // out = call(a) on every polynomial a CKKS ciphertext has (three before relinearization): constants, +-i
    template <typename Call> void elementwise(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o, Call call)
    {
        static_assert(S == Scheme::CKKS, "constants and mult_i / div_i are CKKS operations");
        const int l = limbs(a), parts = a.relinearization_required_ ? 3 : 2;
        require_words(context_, a, parts);
        DeviceVector<Data64> m((size_t) parts * l * context_->n, o.stream_);
        detail::check(call((const uint64_t*) a.data(), (uint64_t*) m.data(), l, parts));
        emit(a, out, std::move(m));
    }
    void constant_op(int op, Ciphertext<S>& a, double value, Ciphertext<S>& out, const ExecutionOptions& o)
    {
        elementwise(a, out, o, [&](const uint64_t* in, uint64_t* m, int l, int parts) {
            return hegpu_ckks_constant_op(context_->handle(), op, in, value, m, l, parts, o.stream_);
        });
    }
    void gaussian(Ciphertext<S>& a, Ciphertext<S>& out, int op, double re, double im, const ExecutionOptions& o)
    {
        elementwise(a, out, o, [&](const uint64_t* in, uint64_t* m, int l, int parts) {
            return hegpu_ckks_gaussian_integer_op(context_->handle(), op, in, re, im, m, l, parts, o.stream_);
        });
    }
    void times_i(Ciphertext<S>& a, Ciphertext<S>& out, int divide, const ExecutionOptions& o)
    {
        elementwise(a, out, o, [&](const uint64_t* in, uint64_t* m, int l, int parts) {
            return hegpu_ckks_mult_i(context_->handle(), in, m, l, parts, divide, o.stream_);
        });
    }
    void plain_addsub(Ciphertext<S>& a, Plaintext<S>& p, Ciphertext<S>& out, int sub, const ExecutionOptions& o)
    {
        if (a.relinearization_required_) throw std::invalid_argument("Ciphertext should be relinearized first!");
        const int l = limbs(a);
        const size_t n = context_->n;
        DeviceVector<Data64> m(2 * n * l, o.stream_);
        if (S == Scheme::CKKS) {
            if (p.depth_ != a.depth_) throw std::logic_error("Ciphertext and Plaintext levels are not equal");
            // part 0 +- plaintext, part 1 unchanged (addition.cu: addition_plain_ckks_poly)
            detail::check(hegpu_addition(context_->handle(), (const uint64_t*) a.data(), (const uint64_t*) p.data(),
                                         (uint64_t*) m.data(), l, 1, 1, sub, o.stream_));
            detail::hip(hipMemcpyAsync(m.data() + n * l, a.data() + n * l, n * l * sizeof(Data64),
                                       hipMemcpyDeviceToDevice, o.stream_));
        } else {
            detail::check(hegpu_bfv_plain_addsub(context_->handle(), (const uint64_t*) a.data(),
                                                 (const uint64_t*) p.data(), (uint64_t*) m.data(), sub, o.stream_));
        }
        emit(a, out, std::move(m));
    }
    HEContext<S> context_;
};

// ------------------------------------------------------------------ N-out-of-N multiparty protocol
// host/{ckks,bfv}/mpcmanager.cuh, util/random.cuh:23-50.  Every party runs a manager of its own next to its secret key;
// the shares travel between parties as the Multiparty* objects below (plain keys with the common seed attached).
//
// RNGSeed: the seed all parties agree on (public).  The reference feeds key / nonce / personalisation string to its
// AES-CTR DRBG; here they are expanded into the 256-bit ChaCha20 key of hegpu_rng_create_seeded: the byte string
//   label || len(key) || key || len(nonce) || nonce || len(pers) || pers        (lengths as 8 bytes, little endian)
// is cut into 32-byte blocks B_0, B_1, ... (zero padded); K_0 = 0, and K_{j+1} = the first 256 bits of the ChaCha20
// stream (hegpu_drbg_block, stream j, indices 0 and 1) under the key K_j xor B_j.  `label` names the kind of key
// ("pk", "rk", "gk" + the Galois element), so that the `a` of one collective key is never reused for another although
// the parties pass the same RNGSeed to all of them.  The result only has to be the same for every party and look
// uniform: the `a` polynomials are public.
struct RNGSeed {
    std::vector<unsigned char> key_, nonce_, personalization_string_;
    RNGSeed() : key_(16), nonce_(8) // 128 + 64 bits from the operating system
    {
        fill(key_);
        fill(nonce_);
    }
    RNGSeed(const std::vector<unsigned char>& key, const std::vector<unsigned char>& nonce,
            const std::vector<unsigned char>& personalization_string)
        : key_(key), nonce_(nonce), personalization_string_(personalization_string)
    {
        if (key_.size() < 16) throw std::invalid_argument("Invalid key size!");
    }
    // the generator of the common polynomials for one kind of key (caller destroys it)
    hegpu_rng* expand(const std::string& label) const
    {
        std::vector<unsigned char> in(label.begin(), label.end());
        for (const auto* part : {&key_, &nonce_, &personalization_string_}) {
            const std::uint64_t len = part->size();
            for (int i = 0; i < 8; i++) in.push_back((unsigned char) (len >> (8 * i)));
            in.insert(in.end(), part->begin(), part->end());
        }
        in.resize((in.size() + 31) / 32 * 32, 0);
        std::uint8_t k[32] = {0};
        for (size_t j = 0; j < in.size() / 32; j++) {
            std::uint8_t x[32];
            for (int i = 0; i < 32; i++) x[i] = k[i] ^ in[32 * j + i];
            std::uint32_t w[8];
            detail::check(hegpu_drbg_block(x, j, 0, w));
            detail::check(hegpu_drbg_block(x, j, 1, w + 4));
            for (int i = 0; i < 32; i++) k[i] = (std::uint8_t) (w[i / 4] >> (8 * (i % 4)));
        }
        hegpu_rng* r = nullptr;
        detail::check(hegpu_rng_create_seeded(k, &r));
        return r;
    }

  private:
    static void fill(std::vector<unsigned char>& v)
    {
        size_t got = 0;
        while (got < v.size()) {
            const ssize_t r = getrandom(v.data() + got, v.size() - got, 0);
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) throw std::runtime_error("getrandom failed");
            got += (size_t) r;
        }
    }
};

template <Scheme S> class MultipartyPublickey : public Publickey<S> { // host/*/publickey.cuh
  public:
    MultipartyPublickey(HEContext<S> context, const RNGSeed seed) : Publickey<S>(std::move(context)), seed_(seed) {}
    inline RNGSeed seed() const noexcept { return seed_; }

  private:
    RNGSeed seed_;
};
template <Scheme S> class MultipartyRelinkey : public Relinkey<S> { // host/*/evaluationkey.cuh
  public:
    MultipartyRelinkey(HEContext<S> context, const RNGSeed seed) : Relinkey<S>(std::move(context)), seed_(seed) {}
    inline RNGSeed seed() const noexcept { return seed_; }

  private:
    RNGSeed seed_;
};
template <Scheme S> class MultipartyGaloiskey : public Galoiskey<S> {
  public:
    MultipartyGaloiskey(HEContext<S> context, const RNGSeed seed) : Galoiskey<S>(std::move(context)), seed_(seed) {}
    MultipartyGaloiskey(HEContext<S> context, std::vector<int>& shift_vec, const RNGSeed seed)
        : Galoiskey<S>(std::move(context), shift_vec), seed_(seed) {}
    MultipartyGaloiskey(HEContext<S> context, std::vector<uint32_t>& galois_elts, const RNGSeed seed)
        : Galoiskey<S>(std::move(context), galois_elts), seed_(seed) {}
    inline RNGSeed seed() const noexcept { return seed_; }

  private:
    RNGSeed seed_;
};

namespace detail {
// what HEMultiPartyManager<CKKS> and <BFV> share: everything but the constructor
template <Scheme S> class MultiPartyManagerBase {
  public:
    ~MultiPartyManagerBase() { hegpu_rng_destroy(rng_); }
    MultiPartyManagerBase(const MultiPartyManagerBase&) = delete;
    MultiPartyManagerBase& operator=(const MultiPartyManagerBase&) = delete;

    void generate_public_key_share(MultipartyPublickey<S>& pk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (pk.public_key_generated_) throw std::logic_error("Publickey is already generated!");
        Crs crs(pk.seed(), "pk");
        DeviceVector<Data64> out((size_t) 2 * context_->Q_prime_size * context_->n, o.stream_);
        Workspace ws(context_->handle(), HEGPU_OP_MPC_KEY_SHARE, 0, o.stream_);
        check(hegpu_mpc_public_key_share(context_->handle(), crs.r, rng_, (const uint64_t*) sk.data(), (uint64_t*) out.data(),
                                         ws.data(), ws.bytes, o.stream_));
        pk.memory_set(std::move(out));
        pk.public_key_generated_ = true;
    }
    void assemble_public_key_share(std::vector<MultipartyPublickey<S>>& all_pk, Publickey<S>& pk,
                                   const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (all_pk.empty()) throw std::invalid_argument("No participant to generate common publickey!");
        std::vector<const uint64_t*> shares;
        for (auto& p : all_pk) {
            if (!p.public_key_generated_) throw std::invalid_argument("MultipartyPublickey is not generated!");
            shares.push_back((const uint64_t*) p.data());
        }
        DeviceVector<Data64> out((size_t) 2 * context_->Q_prime_size * context_->n, o.stream_);
        check(hegpu_mpc_accumulate(context_->handle(), shares.data(), (int) shares.size(), HEGPU_MPC_PUBLIC_KEY,
                                   (uint64_t*) out.data(), o.stream_));
        pk.memory_set(std::move(out));
        pk.public_key_generated_ = true;
    }
    // round 1; the ephemeral secret u stays inside this manager until generate_relin_key_share (the reference keeps
    // the seed that regenerates it, new_seed_)
    void generate_relin_key_init(MultipartyRelinkey<S>& rk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (rk.relin_key_generated_) throw std::logic_error("Relinkey is already generated!");
        Crs crs(rk.seed(), "rk");
        u_ = DeviceVector<Data64>((size_t) context_->Q_prime_size * context_->n, o.stream_);
        DeviceVector<Data64> out(rk.size(), o.stream_);
        Workspace ws(context_->handle(), HEGPU_OP_MPC_KEY_SHARE, 0, o.stream_);
        check(hegpu_mpc_relin_key_share_round1(context_->handle(), crs.r, rng_, (const uint64_t*) sk.data(),
                                               (uint64_t*) u_.data(), (uint64_t*) out.data(), ws.data(), ws.bytes,
                                               o.stream_));
        rk.memory_set(std::move(out));
        rk.relin_key_generated_ = true;
    }
    void assemble_relin_key_init(std::vector<MultipartyRelinkey<S>>& all_rk, MultipartyRelinkey<S>& rk,
                                 const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        std::vector<const uint64_t*> shares = relin_shares(all_rk);
        DeviceVector<Data64> out(rk.size(), o.stream_);
        check(hegpu_mpc_accumulate(context_->handle(), shares.data(), (int) shares.size(), HEGPU_MPC_RELIN_ROUND1,
                                   (uint64_t*) out.data(), o.stream_));
        rk.memory_set(std::move(out));
        rk.relin_key_generated_ = true;
    }
    void generate_relin_key_share(MultipartyRelinkey<S>& rk_s1_common, MultipartyRelinkey<S>& rk_new, Secretkey<S>& sk,
                                  const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (rk_s1_common.key_type != rk_new.key_type) throw std::invalid_argument("Invalid relinkey parameters!");
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (!rk_s1_common.relin_key_generated_) throw std::logic_error("Common Relinkey is not generated!");
        if (rk_new.relin_key_generated_) throw std::logic_error("Relinkey is already generated!");
        if (!u_.size()) throw std::logic_error("generate_relin_key_init has to run first!");
        DeviceVector<Data64> out(rk_new.size(), o.stream_);
        Workspace ws(context_->handle(), HEGPU_OP_MPC_KEY_SHARE, 0, o.stream_);
        check(hegpu_mpc_relin_key_share_round2(context_->handle(), rng_, (const uint64_t*) sk.data(),
                                               (const uint64_t*) u_.data(), (const uint64_t*) rk_s1_common.data(),
                                               (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
        rk_new.memory_set(std::move(out));
        rk_new.relin_key_generated_ = true;
    }
    void assemble_relin_key_share(std::vector<MultipartyRelinkey<S>>& all_rk, MultipartyRelinkey<S>& rk_common_stage1,
                                  Relinkey<S>& rk, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        std::vector<const uint64_t*> shares = relin_shares(all_rk);
        if (!rk_common_stage1.relin_key_generated_) throw std::invalid_argument("MultipartyRelinkey is not generated!");
        DeviceVector<Data64> out(rk.size(), o.stream_);
        check(hegpu_mpc_relin_key_finish(context_->handle(), shares.data(), (int) shares.size(),
                                         (const uint64_t*) rk_common_stage1.data(), (uint64_t*) out.data(), o.stream_));
        rk.memory_set(std::move(out));
        rk.relin_key_generated_ = true;
    }
    void generate_galois_key_share(MultipartyGaloiskey<S>& gk, Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (gk.galois_key_generated_) throw std::logic_error("Galoiskey is already generated!");
        Workspace ws(context_->handle(), HEGPU_OP_MPC_KEY_SHARE, 0, o.stream_);
        for (int elt : elements(gk)) {
            Crs crs(gk.seed(), "gk" + std::to_string(elt));
            DeviceVector<Data64> out(gk.size(), o.stream_);
            check(hegpu_mpc_galois_key_share(context_->handle(), crs.r, rng_, (const uint64_t*) sk.data(), elt,
                                             (uint64_t*) out.data(), ws.data(), ws.bytes, o.stream_));
            gk.device_location_[elt] = std::move(out);
        }
        gk.galois_key_generated_ = true;
    }
    void assemble_galois_key_share(std::vector<MultipartyGaloiskey<S>>& all_gk, Galoiskey<S>& gk,
                                   const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (all_gk.empty()) throw std::invalid_argument("No participant to generate common galois key!");
        for (auto& g : all_gk)
            if (!g.galois_key_generated_) throw std::invalid_argument("MultipartyGaloiskey is not generated!");
        if (gk.galois_key_generated_) throw std::logic_error("Galoiskey is already generated!");
        for (int elt : elements(gk)) {
            std::vector<const uint64_t*> shares;
            for (auto& g : all_gk) {
                shares.push_back(key_for(g, elt));
                if (!shares.back()) throw std::invalid_argument("MultipartyGaloiskey lacks an element!");
            }
            DeviceVector<Data64> out(gk.size(), o.stream_);
            check(hegpu_mpc_accumulate(context_->handle(), shares.data(), (int) shares.size(), HEGPU_MPC_GALOIS_KEY,
                                       (uint64_t*) out.data(), o.stream_));
            gk.device_location_[elt] = std::move(out);
        }
        gk.galois_key_generated_ = true;
    }
    // The reference's shape: a 2-part ciphertext (c0, h_i).  The C ABI produces h_i alone; c0 is copied next to it
    // because callers pass these objects to decrypt(), which reads c0 from the first of them.
    void decrypt_partial(Ciphertext<S>& ciphertext, Secretkey<S>& sk, Ciphertext<S>& partial_ciphertext,
                         const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (ciphertext.size() != 2) throw std::invalid_argument("Ciphertext should be relinearized first!");
        const size_t half = (size_t) (context_->Q_size - ciphertext.depth()) * context_->n;
        DeviceVector<Data64> out(2 * half, o.stream_);
        hip(hipMemcpyAsync(out.data(), ciphertext.data(), half * sizeof(Data64), hipMemcpyDeviceToDevice, o.stream_));
        if (S == Scheme::CKKS)
            check(hegpu_mpc_ckks_decrypt_share(context_->handle(), rng_, (const uint64_t*) ciphertext.data(), 2 * half,
                                               (const uint64_t*) sk.data(), ciphertext.depth(),
                                               (uint64_t*) out.data() + half, 1, o.stream_));
        else
            check(hegpu_mpc_bfv_decrypt_share(context_->handle(), rng_, (const uint64_t*) ciphertext.data(), 2 * half,
                                              (const uint64_t*) sk.data(), (uint64_t*) out.data() + half, 1, o.stream_));
        partial_ciphertext.adopt(std::move(out), 2, ciphertext.depth(), ciphertext.scale());
        partial_ciphertext.encoding_ = ciphertext.encoding_;
    }
    void decrypt(std::vector<Ciphertext<S>>& ciphertexts, Plaintext<S>& plaintext, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (ciphertexts.empty()) throw std::invalid_argument("No ciphertext to decrypt!");
        const int depth = ciphertexts[0].depth();
        for (auto& c : ciphertexts) {
            if (c.depth() != depth) throw std::invalid_argument("Ciphertext levels should be same!");
            if (c.scale() != ciphertexts[0].scale()) throw std::invalid_argument("Ciphertext scales should be same!");
            if (c.encoding_ != ciphertexts[0].encoding_) throw std::invalid_argument("Ciphertext encoding types should be same!");
        }
        const size_t half = (size_t) (context_->Q_size - depth) * context_->n;
        std::vector<const uint64_t*> shares;
        for (auto& c : ciphertexts) shares.push_back((const uint64_t*) c.data() + half);
        const uint64_t* c0 = (const uint64_t*) ciphertexts[0].data();
        DeviceVector<Data64> out(S == Scheme::CKKS ? half : (size_t) context_->n, o.stream_);
        if (S == Scheme::CKKS) {
            check(hegpu_mpc_ckks_decrypt_merge(context_->handle(), c0, 2 * half, shares.data(), (int) shares.size(), depth,
                                               (uint64_t*) out.data(), 1, o.stream_));
        } else {
            Workspace ws(context_->handle(), HEGPU_OP_MPC_BFV_DECRYPT_MERGE, 0, o.stream_);
            check(hegpu_mpc_bfv_decrypt_merge(context_->handle(), c0, 2 * half, shares.data(), (int) shares.size(),
                                              (uint64_t*) out.data(), 1, ws.data(), ws.bytes, o.stream_));
        }
        plaintext.memory_set(std::move(out));
        plaintext.depth_ = depth;
        plaintext.scale_ = ciphertexts[0].scale();
        plaintext.encoding_ = ciphertexts[0].encoding_;
        plaintext.plaintext_generated_ = true;
    }

    // Collective refresh (distributed_bootstrapping_participant / _coordinator, ckks/mpcmanager.cuh:454-560,
    // bfv/mpcmanager.cuh).  The share is a 2-part object as in the reference -- CKKS (h0 over the input's limbs, h1 over
    // all Q), BFV (h0, h1) -- that carries the input's depth and scale; the result is a 2-part ciphertext at depth 0 whose
    // scale and encoding are the input's (the coordinator raises the modulus by an exact integer lift, which changes
    // neither).  The reference's signature has no mask width: bits(Q_level) - 8, capped at 126, leaves room for 64
    // parties (64 * 2^(bits - 9) = Q_level / 8) next to a message below Q_level / 4.
    void distributed_bootstrapping_participant(Ciphertext<S>& common, Ciphertext<S>& output, Secretkey<S>& sk,
                                               const RNGSeed& seed, const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        const DeviceVector<Data64> moved = refresh_input(common, o);
        const uint64_t* ct = moved.size() ? (const uint64_t*) moved.data() : (const uint64_t*) common.data();
        const int Q = context_->Q_size, depth = S == Scheme::CKKS ? common.depth() : 0, l = Q - depth;
        const size_t n = context_->n;
        Crs crs(seed, "boot");
        DeviceVector<Data64> out((size_t) (l + Q) * n, o.stream_);
        if (S == Scheme::CKKS)
            check(hegpu_mpc_ckks_refresh_share(context_->handle(), crs.r, rng_, ct, 2 * l * n, (const uint64_t*) sk.data(), depth,
                                               refresh_mask_bits(l), (uint64_t*) out.data(), 1, nullptr, 0, o.stream_));
        else
            check(hegpu_mpc_bfv_refresh_share(context_->handle(), crs.r, rng_, ct, 2 * l * n, (const uint64_t*) sk.data(),
                                              (uint64_t*) out.data(), 1, nullptr, 0, o.stream_));
        output.adopt(std::move(out), 2, depth, common.scale());
        output.encoding_ = common.encoding_;
    }
    void distributed_bootstrapping_coordinator(std::vector<Ciphertext<S>>& ciphertexts, Ciphertext<S>& common,
                                               Ciphertext<S>& output, const RNGSeed& seed,
                                               const ExecutionOptions& o = ExecutionOptions())
    {
        OpScope storage_scope(o);
        if (ciphertexts.empty()) throw std::invalid_argument("No participant share to refresh with!");
        const DeviceVector<Data64> moved = refresh_input(common, o);
        const uint64_t* ct = moved.size() ? (const uint64_t*) moved.data() : (const uint64_t*) common.data();
        const int Q = context_->Q_size, depth = S == Scheme::CKKS ? common.depth() : 0, l = Q - depth;
        const size_t n = context_->n;
        std::vector<const uint64_t*> shares;
        for (auto& c : ciphertexts) {
            if (c.depth() != depth) throw std::invalid_argument("Ciphertext levels should be same!");
            shares.push_back((const uint64_t*) c.data());
        }
        Crs crs(seed, "boot");
        DeviceVector<Data64> out((size_t) 2 * Q * n, o.stream_);
        Workspace ws(context_->handle(), HEGPU_OP_MPC_REFRESH_MERGE, depth, o.stream_);
        if (S == Scheme::CKKS)
            check(hegpu_mpc_ckks_refresh_merge(context_->handle(), crs.r, ct, 2 * l * n, shares.data(), (int) shares.size(), depth,
                                               (uint64_t*) out.data(), 2 * Q * n, 1, ws.data(), ws.bytes, o.stream_));
        else
            check(hegpu_mpc_bfv_refresh_merge(context_->handle(), crs.r, ct, 2 * l * n, shares.data(), (int) shares.size(),
                                              (uint64_t*) out.data(), 2 * Q * n, 1, ws.data(), ws.bytes, o.stream_));
        const double scale = common.scale();
        const auto encoding = common.encoding_;
        output.adopt(std::move(out), 2, 0, scale);
        output.encoding_ = encoding;
    }

  protected:
    explicit MultiPartyManagerBase(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
        check(hegpu_rng_create_from_entropy(&rng_)); // the party's private generator
    }

  private:
    struct Crs { // the common generator of one key, from the seed the key carries
        Crs(const RNGSeed& seed, const std::string& label) : r(seed.expand(label)) {}
        ~Crs() { hegpu_rng_destroy(r); }
        Crs(const Crs&) = delete;
        Crs& operator=(const Crs&) = delete;
        hegpu_rng* r;
    };
    // the checks of a refresh input (the evaluator's exception class for such inputs); a coefficient-domain CKKS
    // ciphertext comes back transformed (an empty vector: use the ciphertext's own residues)
    DeviceVector<Data64> refresh_input(Ciphertext<S>& ct, const ExecutionOptions& o)
    {
        if (ct.relinearization_required() || ct.size() != 2) throw std::invalid_argument("Ciphertext should be relinearized first!");
        if (ct.rescale_required()) throw std::invalid_argument("Ciphertext should be rescaled first!");
        if (S != Scheme::CKKS || ct.in_ntt_domain()) return DeviceVector<Data64>();
        const int l = context_->Q_size - ct.depth();
        DeviceVector<Data64> t((size_t) 2 * l * context_->n, o.stream_);
        check(hegpu_ntt(context_->handle(), HEGPU_TABLES_QP, (const uint64_t*) ct.data(), (uint64_t*) t.data(), 0, 2 * l, l, 0,
                        nullptr, nullptr, o.stream_));
        return t;
    }
    int refresh_mask_bits(int l) const
    {
        // a product of l numbers of b_i bits has at least sum b_i - (l - 1) bits: the lower bound keeps the mask legal
        int bits = -(l - 1);
        for (int i = 0; i < l; i++) bits += (int) context_->prime_vector_[i].bit;
        return bits - 8 > 126 ? 126 : bits - 8;
    }
    static std::vector<const uint64_t*> relin_shares(std::vector<MultipartyRelinkey<S>>& all_rk)
    {
        if (all_rk.empty()) throw std::invalid_argument("No participant to generate common relinkey!");
        std::vector<const uint64_t*> shares;
        for (auto& r : all_rk) {
            if (!r.relin_key_generated_) throw std::invalid_argument("MultipartyRelinkey is not generated!");
            shares.push_back((const uint64_t*) r.data());
        }
        return shares;
    }
    static std::vector<int> elements(const Galoiskey<S>& gk) // the listed elements and the column-rotation key, each once
    {
        std::vector<int> e;
        if (gk.customized) for (std::uint32_t x : gk.custom_galois_elt) e.push_back((int) x);
        else for (const auto& g : gk.galois_elt) e.push_back(g.second);
        e.push_back(gk.galois_elt_zero);
        std::sort(e.begin(), e.end());
        e.erase(std::unique(e.begin(), e.end()), e.end());
        return e;
    }
    HEContext<S> context_;
    hegpu_rng* rng_ = nullptr;
    DeviceVector<Data64> u_; // round 1 -> round 2 of the relinearisation key
};
} // namespace detail

template <Scheme S> class HEMultiPartyManager;
template <> class HEMultiPartyManager<Scheme::CKKS> : public detail::MultiPartyManagerBase<Scheme::CKKS> {
  public:
    // encoder and scale serve the reference's collective bootstrapping, which re-encodes at the manager's scale; here
    // the refresh is an integer lift that keeps the ciphertext's own scale, and neither is needed
    HEMultiPartyManager(HEContext<Scheme::CKKS> context, HEEncoder<Scheme::CKKS>&, double&)
        : detail::MultiPartyManagerBase<Scheme::CKKS>(std::move(context)) {}
};
template <> class HEMultiPartyManager<Scheme::BFV> : public detail::MultiPartyManagerBase<Scheme::BFV> {
  public:
    explicit HEMultiPartyManager(HEContext<Scheme::BFV> context) : detail::MultiPartyManagerBase<Scheme::BFV>(std::move(context)) {}
};

// ------------------------------------------------------------------ TFHE (host/tfhe/*.cuh)
// Fixed parameter set (tfhe/context.cu:15-57).  Ciphertexts are LWE samples a [shape][n], b [shape]
// on the 32-bit torus; a bit is +-1/8.
template <> class HEContextImpl<Scheme::TFHE> {
  public:
    explicit HEContextImpl(sec_level_type = sec_level_type::sec128)
    {
        detail::check(hegpu_tfhe_context_create(&h_));
        n_ = (int) hegpu_tfhe_context_int(h_, "n");
        N_ = (int) hegpu_tfhe_context_int(h_, "N");
        k_ = (int) hegpu_tfhe_context_int(h_, "k");
    }
    ~HEContextImpl() { if (h_) hegpu_tfhe_context_destroy(h_); }
    HEContextImpl(const HEContextImpl&) = delete;
    hegpu_tfhe_context* handle() const { return h_; }
    long elems(const char* what) const { return hegpu_tfhe_context_int(h_, what); }
    int n_ = 0, N_ = 0, k_ = 0;
    bool context_generated_ = true;

  private:
    hegpu_tfhe_context* h_ = nullptr;
};

template <> class Ciphertext<Scheme::TFHE> {
  public:
    explicit Ciphertext(HEContext<Scheme::TFHE> context, const ExecutionOptions& = ExecutionOptions())
    {
        detail::require_generated(context);
        n_ = context->n_;
    }
    DeviceVector<int32_t> a_device_location_, b_device_location_;
    int n_ = 0, shape_ = 0;
    bool ciphertext_generated_ = false;
};

template <> class Secretkey<Scheme::TFHE> {
  public:
    explicit Secretkey(HEContext<Scheme::TFHE> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
    DeviceVector<int32_t> lwe_key_device_location_, tlwe_key_device_location_;
    bool secret_key_generated_ = false;

  private:
    HEContext<Scheme::TFHE> context_;
};

template <Scheme S> class Bootstrappingkey;
template <> class Bootstrappingkey<Scheme::TFHE> { // boot key (prepared for the blind rotate) + key-switch key
  public:
    explicit Bootstrappingkey(HEContext<Scheme::TFHE> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
    DeviceVector<Data64> boot_key_device_location_;  // reference layout [n][k+1][l][k+1][N], NTT domain
    DeviceVector<Data64> prepared_;                  // hegpu_tfhe_prepare_bootkey
    DeviceVector<int32_t> switch_key_device_location_a_, switch_key_device_location_b_;
    bool boot_key_generated_ = false;

  private:
    HEContext<Scheme::TFHE> context_;
};

template <> class HEKeyGenerator<Scheme::TFHE> { // host/tfhe/keygenerator.cuh
    static constexpr Scheme S = Scheme::TFHE;

  public:
    explicit HEKeyGenerator(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
        detail::check(hegpu_rng_create_from_entropy(&rng_));
    }
    // REPRODUCIBLE TESTS ONLY (64-bit seed)
    HEKeyGenerator(HEContext<S> context, std::uint64_t seed) : context_(std::move(context))
    {
        detail::require_generated(context_);
        detail::check(hegpu_rng_create(seed, &rng_));
    }
    ~HEKeyGenerator() { hegpu_rng_destroy(rng_); }
    HEKeyGenerator(const HEKeyGenerator&) = delete;
    HEKeyGenerator& operator=(const HEKeyGenerator&) = delete;

    void generate_secret_key(Secretkey<S>& sk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (sk.secret_key_generated_) throw std::logic_error("Secretkey is already generated!");
        sk.lwe_key_device_location_ = DeviceVector<int32_t>((size_t) context_->n_, o.stream_);
        sk.tlwe_key_device_location_ = DeviceVector<int32_t>((size_t) context_->k_ * context_->N_, o.stream_);
        detail::check(hegpu_tfhe_generate_secret_key(context_->handle(), rng_, sk.lwe_key_device_location_.data(),
                                                     sk.tlwe_key_device_location_.data(), o.stream_));
        sk.secret_key_generated_ = true;
    }
    void generate_bootstrapping_key(Bootstrappingkey<S>& bk, Secretkey<S>& sk,
                                    const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        if (bk.boot_key_generated_) throw std::logic_error("Bootstrappingkey is already generated!");
        bk.boot_key_device_location_ = DeviceVector<Data64>((size_t) context_->elems("bootkey_elems"), o.stream_);
        bk.switch_key_device_location_a_ = DeviceVector<int32_t>((size_t) context_->elems("kskey_a_elems"), o.stream_);
        bk.switch_key_device_location_b_ = DeviceVector<int32_t>((size_t) context_->elems("kskey_b_elems"), o.stream_);
        DeviceVector<Data64> ws((size_t) context_->N_, o.stream_);
        detail::check(hegpu_tfhe_generate_bootstrapping_key(
            context_->handle(), rng_, sk.lwe_key_device_location_.data(), sk.tlwe_key_device_location_.data(),
            (uint64_t*) bk.boot_key_device_location_.data(), bk.switch_key_device_location_a_.data(),
            bk.switch_key_device_location_b_.data(), ws.data(), ws.size() * sizeof(Data64), o.stream_));
        bk.prepared_ = DeviceVector<Data64>((size_t) context_->elems("prepared_bootkey_elems"), o.stream_);
        detail::check(hegpu_tfhe_prepare_bootkey(context_->handle(), (const uint64_t*) bk.boot_key_device_location_.data(),
                                                 (uint64_t*) bk.prepared_.data(), o.stream_));
        bk.boot_key_generated_ = true;
    }

  private:
    HEContext<S> context_;
    hegpu_rng* rng_ = nullptr;
};

template <> class HEEncryptor<Scheme::TFHE> { // host/tfhe/encryptor.cuh: symmetric LWE encryption of bits
    static constexpr Scheme S = Scheme::TFHE;

  public:
    HEEncryptor(HEContext<S> context, Secretkey<S>& sk) : context_(std::move(context)), sk_(&sk)
    {
        detail::require_generated(context_);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
        detail::check(hegpu_rng_create_from_entropy(&rng_));
    }
    ~HEEncryptor() { hegpu_rng_destroy(rng_); }
    HEEncryptor(const HEEncryptor&) = delete;
    HEEncryptor& operator=(const HEEncryptor&) = delete;

    void encrypt(Ciphertext<S>& ct, const std::vector<bool>& messages, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        const int shape = (int) messages.size();
        std::vector<int32_t> enc(messages.size());
        for (size_t i = 0; i < messages.size(); i++) enc[i] = messages[i] ? (1 << 29) : -(1 << 29); // +-1/8
        DeviceVector<int32_t> msg(enc, o.stream_);
        ct.a_device_location_ = DeviceVector<int32_t>((size_t) shape * context_->n_, o.stream_);
        ct.b_device_location_ = DeviceVector<int32_t>((size_t) shape, o.stream_);
        detail::check(hegpu_tfhe_encrypt(context_->handle(), rng_, sk_->lwe_key_device_location_.data(), msg.data(),
                                         shape, ct.a_device_location_.data(), ct.b_device_location_.data(), o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
        ct.shape_ = shape;
        ct.ciphertext_generated_ = true;
    }

  private:
    HEContext<S> context_;
    Secretkey<S>* sk_;
    hegpu_rng* rng_ = nullptr;
};

template <> class HEDecryptor<Scheme::TFHE> { // host/tfhe/decryptor.cuh
    static constexpr Scheme S = Scheme::TFHE;

  public:
    HEDecryptor(HEContext<S> context, Secretkey<S>& sk) : context_(std::move(context)), sk_(&sk)
    {
        detail::require_generated(context_);
        if (!sk.secret_key_generated_) throw std::logic_error("Secretkey is not generated!");
    }
    void decrypt(Ciphertext<S>& ct, std::vector<bool>& messages, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        DeviceVector<int32_t> phase((size_t) ct.shape_, o.stream_);
        detail::check(hegpu_tfhe_decrypt_phase(context_->handle(), sk_->lwe_key_device_location_.data(),
                                               ct.a_device_location_.data(), ct.b_device_location_.data(), ct.shape_,
                                               phase.data(), o.stream_));
        std::vector<int32_t> h((size_t) ct.shape_);
        detail::hip(hipMemcpyAsync(h.data(), phase.data(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, o.stream_));
        detail::hip(hipStreamSynchronize(o.stream_));
        messages.resize(h.size());
        for (size_t i = 0; i < h.size(); i++) messages[i] = h[i] > 0;
    }

  private:
    HEContext<S> context_;
    Secretkey<S>* sk_;
};

template <Scheme S> class HELogicOperator;
template <> class HELogicOperator<Scheme::TFHE> { // host/tfhe/operator.cuh: bootstrapped binary gates
    static constexpr Scheme S = Scheme::TFHE;

  public:
    explicit HELogicOperator(HEContext<S> context) : context_(std::move(context))
    {
        detail::require_generated(context_);
    }
#define HEONGPU_TFHE_GATE(NAME, ID)                                                                              \
    void NAME(Ciphertext<S>& in1, Ciphertext<S>& in2, Ciphertext<S>& out, Bootstrappingkey<S>& bk,               \
              const ExecutionOptions& o = ExecutionOptions())                                                    \
    {                                                                                                            \
        gate(ID, in1, in2, out, bk, o);                                                                          \
    }
    HEONGPU_TFHE_GATE(NAND, HEGPU_GATE_NAND)
    HEONGPU_TFHE_GATE(AND, HEGPU_GATE_AND)
    HEONGPU_TFHE_GATE(NOR, HEGPU_GATE_NOR)
    HEONGPU_TFHE_GATE(OR, HEGPU_GATE_OR)
    HEONGPU_TFHE_GATE(XNOR, HEGPU_GATE_XNOR)
    HEONGPU_TFHE_GATE(XOR, HEGPU_GATE_XOR)
#undef HEONGPU_TFHE_GATE
    void NOT(Ciphertext<S>& in, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (!in.ciphertext_generated_) throw std::runtime_error("Input is not generated!");
        DeviceVector<int32_t> a((size_t) in.shape_ * context_->n_, o.stream_), b((size_t) in.shape_, o.stream_);
        detail::check(hegpu_tfhe_gate_precompute(context_->handle(), HEGPU_GATE_NOT, a.data(), b.data(),
                                                 in.a_device_location_.data(), in.b_device_location_.data(), nullptr,
                                                 nullptr, in.shape_, o.stream_));
        finish(out, in.shape_, std::move(a), std::move(b));
    }
    void MUX(Ciphertext<S>& in1, Ciphertext<S>& in2, Ciphertext<S>& control, Ciphertext<S>& out,
             Bootstrappingkey<S>& bk, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        if (in1.shape_ != in2.shape_ || in1.shape_ != control.shape_)
            throw std::runtime_error("Ciphertexts size should be equal!");
        if (!(in1.ciphertext_generated_ && in2.ciphertext_generated_)) throw std::runtime_error("One or the inputs are generated!");
        const int shape = in1.shape_;
        DeviceVector<int32_t> a((size_t) shape * context_->n_, o.stream_), b((size_t) shape, o.stream_);
        DeviceVector<int32_t> ws(((size_t) context_->n_ + 1 + 2 * ((size_t) context_->k_ * context_->N_ + 1)) * shape,
                                 o.stream_);
        detail::check(hegpu_tfhe_mux(context_->handle(), in1.a_device_location_.data(), in1.b_device_location_.data(),
                                     in2.a_device_location_.data(), in2.b_device_location_.data(),
                                     control.a_device_location_.data(), control.b_device_location_.data(), a.data(),
                                     b.data(), (const uint64_t*) bk.prepared_.data(),
                                     bk.switch_key_device_location_a_.data(), bk.switch_key_device_location_b_.data(),
                                     shape, ws.data(), ws.size() * sizeof(int32_t), o.stream_));
        finish(out, shape, std::move(a), std::move(b));
    }

  private:
    void gate(int id, Ciphertext<S>& in1, Ciphertext<S>& in2, Ciphertext<S>& out, Bootstrappingkey<S>& bk,
              const ExecutionOptions& o)
    {
        if (in1.shape_ != in2.shape_) throw std::runtime_error("Ciphertexts size should be equal!");
        if (!(in1.ciphertext_generated_ && in2.ciphertext_generated_)) throw std::runtime_error("One or the inputs are generated!");
        if (!bk.boot_key_generated_) throw std::runtime_error("Bootstrappingkey is not generated!");
        const int shape = in1.shape_;
        DeviceVector<int32_t> a((size_t) shape * context_->n_, o.stream_), b((size_t) shape, o.stream_);
        DeviceVector<int32_t> ws(((size_t) context_->n_ + (size_t) context_->k_ * context_->N_ + 2) * shape, o.stream_);
        detail::check(hegpu_tfhe_gate(context_->handle(), id, in1.a_device_location_.data(),
                                      in1.b_device_location_.data(), in2.a_device_location_.data(),
                                      in2.b_device_location_.data(), a.data(), b.data(),
                                      (const uint64_t*) bk.prepared_.data(), bk.switch_key_device_location_a_.data(),
                                      bk.switch_key_device_location_b_.data(), shape, ws.data(),
                                      ws.size() * sizeof(int32_t), o.stream_));
        finish(out, shape, std::move(a), std::move(b));
    }
    void finish(Ciphertext<S>& out, int shape, DeviceVector<int32_t>&& a, DeviceVector<int32_t>&& b)
    {
        out.a_device_location_ = std::move(a);
        out.b_device_location_ = std::move(b);
        out.shape_ = shape;
        out.n_ = context_->n_;
        out.ciphertext_generated_ = true;
    }
    HEContext<S> context_;
};

// ------------------------------------------------------------------ logic gates on encrypted bits, BFV and CKKS
// HELogicOperator<Scheme::BFV> (host/bfv/operator.cuh:1324-2230) and HELogicOperator<Scheme::CKKS>
// (host/ckks/operator.cuh:2333-3500): a bit is the value 0 or 1 in a slot and a gate is c0 + c1 (a + b) + c2 (a b).
// Every gate is one hegpu_{bfv,ckks}_logic_gate call: the product sequence of the arithmetic operator, then ONE pass that
// reads a, b and the product in place (the reference chains add, add, mod_drop, sub, negate and a plaintext add, each
// "TODO: make it efficient").  Three deliberate departures from the reference:
//  1. Its CKKS ciphertext-ciphertext OR, XOR, NOR and XNOR hand a depth-d sum and a depth-d+1 product to sub(), which
//     throws "Ciphertexts leveled are not equal"; only some plaintext variants mod_drop first.  Here every gate reads the
//     sum at the product's level, so all of them work and leave at depth + 1.
//  2. Its out-of-place one_minus_cipher (ckks/operator.cu:7329-7346, bfv/operator.cu:1520-1575) negates its INPUT in
//     place.  Here inputs are never modified.
//  3. Of the bootstrapped members, generate_bootstrapping_params, bootstrapping_key_indexs, bit_bootstrapping,
//     gate_bootstrapping and the six *_bootstrapping gates are provided on the parts of the regular refresh (DESIGN.md
//     4.5g).  The *_approximation gates are not declared: they take a mid-pipeline ciphertext that does not exist here.
namespace detail {
template <Scheme S> class LogicOperatorBase {
  public:
    void NOT(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o); // storage manager: stage HOST-stored operands, place the results
        gate(HEGPU_LOGIC_NOT, a, nullptr, nullptr, nullptr, out, o);
    }
    void NOT_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions())
    {
        detail::OpScope storage_scope(o);
        gate(HEGPU_LOGIC_NOT, a, nullptr, nullptr, nullptr, a, o);
    }
    // the four forms of a binary gate: (ct, ct, out, relin_key), _inplace(ct, ct, relin_key), (ct, pt, out), _inplace(ct, pt)
#define HEONGPU_LOGIC_GATE_FORMS(NAME)                                                                                     \
    void NAME(Ciphertext<S>& a, Ciphertext<S>& b, Ciphertext<S>& out, Relinkey<S>& rk,                                     \
              const ExecutionOptions& o = ExecutionOptions())                                                              \
    {                                                                                                                      \
        detail::OpScope storage_scope(o);                                                                                  \
        gate(HEGPU_LOGIC_##NAME, a, &b, nullptr, &rk, out, o);                                                             \
    }                                                                                                                      \
    void NAME##_inplace(Ciphertext<S>& a, Ciphertext<S>& b, Relinkey<S>& rk, const ExecutionOptions& o = ExecutionOptions()) \
    {                                                                                                                      \
        detail::OpScope storage_scope(o);                                                                                  \
        gate(HEGPU_LOGIC_##NAME, a, &b, nullptr, &rk, a, o);                                                               \
    }                                                                                                                      \
    void NAME(Ciphertext<S>& a, Plaintext<S>& b, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions())       \
    {                                                                                                                      \
        detail::OpScope storage_scope(o);                                                                                  \
        gate(HEGPU_LOGIC_##NAME, a, nullptr, &b, nullptr, out, o);                                                         \
    }                                                                                                                      \
    void NAME##_inplace(Ciphertext<S>& a, Plaintext<S>& b, const ExecutionOptions& o = ExecutionOptions())                 \
    {                                                                                                                      \
        detail::OpScope storage_scope(o);                                                                                  \
        gate(HEGPU_LOGIC_##NAME, a, nullptr, &b, nullptr, a, o);                                                           \
    }
    HEONGPU_LOGIC_GATE_FORMS(AND)
    HEONGPU_LOGIC_GATE_FORMS(OR)
    HEONGPU_LOGIC_GATE_FORMS(XOR)
    HEONGPU_LOGIC_GATE_FORMS(NAND)
    HEONGPU_LOGIC_GATE_FORMS(NOR)
    HEONGPU_LOGIC_GATE_FORMS(XNOR)
#undef HEONGPU_LOGIC_GATE_FORMS

  protected:
    LogicOperatorBase(HEContext<S> context, double scale_one) : context_(std::move(context)), scale_one_(scale_one)
    {
        detail::require_generated(context_);
    }
    HEContext<S> context_;
    double scale_one_; // CKKS: the scale at which the constant one enters (the reference's encoded_constant_one_)

  private:
    // the checks and exception types of the arithmetic operator's multiply / multiply_plain / add
    void check_cipher(const Ciphertext<S>& c) const
    {
        if (c.relinearization_required_ || c.cipher_size_ != 2)
            throw std::invalid_argument("Ciphertexts can not be used because of the non-linear part! Please use "
                                        "relinearization operation!");
        if (c.rescale_required_)
            throw std::invalid_argument("Ciphertexts can not be used because of the noise! Please use rescale operation to "
                                        "get rid of additional noise!");
        if (S == Scheme::BFV && c.in_ntt_domain_) throw std::invalid_argument("Ciphertext should be in intt domain");
        HEArithmeticOperator<S>::require_words(context_, c, 2);
    }
    void gate(int g, Ciphertext<S>& a, Ciphertext<S>* bc, Plaintext<S>* bp, Relinkey<S>* rk, Ciphertext<S>& out,
              const ExecutionOptions& o)
    {
        constexpr bool ckks = S == Scheme::CKKS;
        const bool unary = g == HEGPU_LOGIC_NOT;
        const int l = context_->Q_size - a.depth_;
        const size_t n = context_->n;
        check_cipher(a);
        if (bc) {
            if (a.depth_ != bc->depth_) throw std::logic_error("Ciphertexts leveled are not equal");
            check_cipher(*bc); // at a's level: the depths are equal
        }
        if (bp) {
            if (ckks && bp->depth_ != a.depth_) throw std::logic_error("Ciphertext and Plaintext levels are not equal");
            if (!ckks && bp->in_ntt_domain_)
                throw std::logic_error("BFV ciphertext or plaintext should be not in same domain");
            if (bp->size() < (ckks ? n * l : n)) throw std::invalid_argument("Invalid plaintext size!");
        }
        if (ckks && !unary && l < 2)
            throw std::logic_error("Ciphertext modulus can not be reducible, since there is only one modulus");
        const int out_limbs = (ckks && !unary) ? l - 1 : l;
        const int kind = bc ? HEGPU_GATE_B_CIPHER : bp ? HEGPU_GATE_B_PLAIN : HEGPU_GATE_B_NONE;
        const uint64_t* b = bc ? (const uint64_t*) bc->data() : bp ? (const uint64_t*) bp->data() : nullptr;
        const uint64_t* key = rk ? (const uint64_t*) rk->data() : nullptr;
        // fresh memory for every result, in place too: the limb count of a CKKS binary gate changes
        DeviceVector<Data64> m((size_t) 2 * out_limbs * n, o.stream_);
        const int op = ckks ? HEGPU_OP_CKKS_LOGIC_GATE : HEGPU_OP_BFV_LOGIC_GATE;
        detail::Workspace ws(unary ? 0 : hegpu_workspace_bytes(context_->handle(), op, a.depth_, 1), o.stream_); // NOT: none
        if (ckks)
            detail::check(hegpu_ckks_logic_gate(context_->handle(), g, (const uint64_t*) a.data(), 0, b, kind, 0, key,
                                                scale_one_, (uint64_t*) m.data(), 0, a.depth_, 1, ws.data(), ws.bytes,
                                                o.stream_));
        else
            detail::check(hegpu_bfv_logic_gate(context_->handle(), g, (const uint64_t*) a.data(), 0, b, kind, 0, key,
                                               (uint64_t*) m.data(), 0, 1, ws.data(), ws.bytes, o.stream_));
        // AND / NAND leave at the product's scale; the other gates at the first operand's, as the reference's last sub
        // leaves it.  (In place: a's fields are read before they are written.)
        double sc = a.scale_;
        if (ckks && (g == HEGPU_LOGIC_AND || g == HEGPU_LOGIC_NAND))
            sc = a.scale_ * (bc ? bc->scale_ : bp->scale_) / (double) context_->prime_vector_[l - 1].value;
        const int depth = a.depth_ + ((ckks && !unary) ? 1 : 0);
        out.encoding_ = a.encoding_;
        HEArithmeticOperator<S>::emit(a, out, std::move(m)); // two parts, no pending rescale or relinearization: check_cipher(a)
        out.depth_ = depth;
        out.scale_ = sc;
    }
};
} // namespace detail

template <> class HELogicOperator<Scheme::BFV> : public detail::LogicOperatorBase<Scheme::BFV> {
  public:
    HELogicOperator(HEContext<Scheme::BFV> context, HEEncoder<Scheme::BFV>&) : LogicOperatorBase(std::move(context), 0.0) {}
};

template <> class HELogicOperator<Scheme::CKKS> : public detail::LogicOperatorBase<Scheme::CKKS> {
    static constexpr Scheme S = Scheme::CKKS;

  public:
    HELogicOperator(HEContext<S> context, HEEncoder<S>&, double scale)
        : LogicOperatorBase(std::move(context), scale), arithmetic_(context_)
    {
        if (scale == 0.0) throw std::invalid_argument("Scale can not be zero for CKKS logic operator.");
    }
    // the reference's class reaches these through its private base (example/basic/12_basic_ckks_logic.cpp calls
    // mod_drop_inplace on a plaintext): the arithmetic operator's implementation, not a copy of it
    void mod_drop(Ciphertext<S>& a, Ciphertext<S>& out, const ExecutionOptions& o = ExecutionOptions()) { arithmetic_.mod_drop(a, out, o); }
    void mod_drop_inplace(Ciphertext<S>& a, const ExecutionOptions& o = ExecutionOptions()) { arithmetic_.mod_drop_inplace(a, o); }
    void mod_drop(Plaintext<S>& p, Plaintext<S>& out, const ExecutionOptions& o = ExecutionOptions()) { arithmetic_.mod_drop(p, out, o); }
    void mod_drop_inplace(Plaintext<S>& p, const ExecutionOptions& o = ExecutionOptions()) { arithmetic_.mod_drop_inplace(p, o); }


    // ---- bit and gate bootstrapping (host/ckks/operator.cuh:3255-3449, eprint 2024/767): the slim
    // sequence of the arithmetic operator with ratio 2 (bit) or 3 (gates) and the function's cosine.  The reference's
    // checks and texts are kept; its departures are HEArithmeticOperator::generate_bootstrapping_params's.  The
    // *_approximation members stay undeclared: they take a mid-pipeline ciphertext that does not exist here.
    // set_chained_giant_steps: the arithmetic operator's switch (the reduced Galois key set), read by the call below
    void set_chained_giant_steps(bool on) noexcept { arithmetic_.set_chained_giant_steps(on); }
    bool chained_giant_steps() const noexcept { return arithmetic_.chained_giant_steps(); }
    void generate_bootstrapping_params(const double scale, const BootstrappingConfig& config,
                                       const logic_bootstrapping_type& boot_type)
    {
        if (arithmetic_.slim_family_generated())
            throw std::runtime_error("Bootstrapping parameters is locked after generation and cannot be modified.");
        const int division = static_cast<int>(std::round(static_cast<double>(context_->prime_vector_[0].value) / scale));
        switch (static_cast<int>(boot_type)) {
            case 1: // BIT_BOOTSTRAPPING
                if (division != 2)
                    throw std::invalid_argument("Bootstrapping parameters can not be generated, because of context is not "
                                                "suitable for Bit Bootstrapping. Last modulus should be 2*scale!");
                break;
            case 2: // GATE_BOOTSTRAPPING
                if (division != 3)
                    throw std::invalid_argument("Bootstrapping parameters can not be generated, because of context is not "
                                                "suitable for Gate Bootstrapping. Last modulus should be 3*scale!");
                break;
            default:
                throw std::invalid_argument("Invalid Bootstrapping Type");
        }
        arithmetic_.generate_slim_family_params(scale, config, (double) division, false);
        boot_type_ = boot_type;
    }
    std::vector<int> bootstrapping_key_indexs()
    {
        if (!arithmetic_.slim_family_generated())
            throw std::invalid_argument("Bootstrapping key indexs can not be returned before generating Bootstrapping parameters!");
        return arithmetic_.bootstrapping_key_indexs();
    }
    Ciphertext<S> bit_bootstrapping(Ciphertext<S>& input1, Galoiskey<S>& galois_key, Relinkey<S>& relin_key,
                                    const ExecutionOptions& options = ExecutionOptions())
    {
        if (boot_type_ != logic_bootstrapping_type::BIT_BOOTSTRAPPING)
            throw std::invalid_argument("Bootstrapping operation can not be performed before generating Bootstrapping parameters!");
        return arithmetic_.slim_family_bootstrapping(HEArithmeticOperator<S>::BIT_FUNCTION, input1, nullptr, galois_key, relin_key,
                                                     options);
    }
#define HEONGPU_GATE_BOOTSTRAPPING(NAME)                                                                                   \
    Ciphertext<S> NAME##_bootstrapping(Ciphertext<S>& input1, Ciphertext<S>& input2, Galoiskey<S>& galois_key,             \
                                       Relinkey<S>& relin_key, const ExecutionOptions& options = ExecutionOptions())       \
    {                                                                                                                      \
        return gate_bootstrapping(logic_gate::NAME, input1, input2, galois_key, relin_key, options);                      \
    }
    HEONGPU_GATE_BOOTSTRAPPING(AND)
    HEONGPU_GATE_BOOTSTRAPPING(OR)
    HEONGPU_GATE_BOOTSTRAPPING(XOR)
    HEONGPU_GATE_BOOTSTRAPPING(NAND)
    HEONGPU_GATE_BOOTSTRAPPING(NOR)
    HEONGPU_GATE_BOOTSTRAPPING(XNOR)
#undef HEONGPU_GATE_BOOTSTRAPPING

  private:
    enum class logic_gate { AND, OR, XOR, NAND, NOR, XNOR };
    Ciphertext<S> gate_bootstrapping(logic_gate gate_type, Ciphertext<S>& input1, Ciphertext<S>& input2, Galoiskey<S>& galois_key,
                                     Relinkey<S>& relin_key, const ExecutionOptions& options = ExecutionOptions())
    {
        if (boot_type_ != logic_bootstrapping_type::GATE_BOOTSTRAPPING)
            throw std::invalid_argument("Bootstrapping operation can not be performed before generating Bootstrapping parameters!");
        return arithmetic_.slim_family_bootstrapping(HEArithmeticOperator<S>::AND_FUNCTION + static_cast<int>(gate_type), input1,
                                                     &input2, galois_key, relin_key, options);
    }
    HEArithmeticOperator<S> arithmetic_;
    logic_bootstrapping_type boot_type_ = logic_bootstrapping_type::NONE;
};

// ------------------------------------------------------------------ serializer (util/serializer.h:20-131)
// file = u64 size + zlib stream of the object's save() bytes
namespace serializer {
inline std::vector<std::uint8_t> to_buffer(const std::stringstream& ss)
{
    const std::string str = ss.str();
    return {str.begin(), str.end()};
}
inline void from_buffer(std::stringstream& ss, const std::vector<std::uint8_t>& buffer)
{
    ss.str(std::string(buffer.begin(), buffer.end()));
}
#if defined(HEONGPU_WITH_ZLIB)
inline std::vector<std::uint8_t> compress(const std::vector<std::uint8_t>& data)
{
    uLongf bound = compressBound(data.size());
    std::vector<std::uint8_t> out(bound);
    if (::compress(out.data(), &bound, data.data(), data.size()) != Z_OK)
        throw std::runtime_error("Zlib compression failed");
    out.resize(bound);
    return out;
}
inline std::vector<std::uint8_t> decompress(const std::vector<std::uint8_t>& data)
{
    // the reference sizes the output at 4x the input and fails beyond; grow instead
    for (size_t factor = 4; factor <= 4096; factor *= 4) {
        std::vector<std::uint8_t> out(data.size() * factor + 64);
        uLongf out_size = out.size();
        const int rc = ::uncompress(out.data(), &out_size, data.data(), data.size());
        if (rc == Z_OK) {
            out.resize(out_size);
            return out;
        }
        if (rc != Z_BUF_ERROR) break;
    }
    throw std::runtime_error("Zlib decompression failed");
}
template <typename T> std::vector<std::uint8_t> serialize(const T& obj)
{
    std::stringstream ss;
    obj.save(ss);
    return compress(to_buffer(ss));
}
// the object is constructed by the caller (it needs its context)
template <typename T> void deserialize(T& obj, const std::vector<std::uint8_t>& buffer)
{
    std::stringstream ss;
    from_buffer(ss, decompress(buffer));
    obj.load(ss);
}
// reference signature (util/serializer.h:86): objects that can be default-constructed
template <typename T> T deserialize(const std::vector<std::uint8_t>& buffer)
{
    T obj;
    deserialize(obj, buffer);
    return obj;
}
template <typename T> void save_to_file(const T& obj, const std::string& filename)
{
    const std::vector<std::uint8_t> data = serialize(obj);
    const std::uint64_t size = data.size();
    std::ofstream ofs(filename, std::ios::binary);
    if (!ofs) throw std::runtime_error("Cannot open file for writing: " + filename);
    ofs.write((const char*) &size, sizeof(size));
    ofs.write((const char*) data.data(), (std::streamsize) size);
}
template <typename T> void load_from_file(T& obj, const std::string& filename)
{
    std::ifstream ifs(filename, std::ios::binary);
    if (!ifs) throw std::runtime_error("Cannot open file for reading: " + filename);
    std::uint64_t size = 0;
    ifs.read((char*) &size, sizeof(size));
    std::vector<std::uint8_t> buffer(size);
    ifs.read((char*) buffer.data(), (std::streamsize) size);
    if (!ifs) throw std::runtime_error("File is truncated: " + filename);
    deserialize(obj, buffer);
}
template <typename T> T load_from_file(const std::string& filename) // util/serializer.h:115
{
    T obj;
    load_from_file(obj, filename);
    return obj;
}
#endif // HEONGPU_WITH_ZLIB
} // namespace serializer

} // namespace heongpu
