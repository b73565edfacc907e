// host_call.hip -- the single calls of the C-ABI on host pointers (include/sprintz_mi355x.h): the drop-in symbols of the
// reference's signatures, their layout / header-less / run-less forms, the single-call queries and the chunked host
// convenience pair.  The thread's pooled scratch, the ticket and event waits and the staging kernel live here; the only
// host-side stream logic is the framing walk that sizes the H2D copy of the length-less reference decompress() signature.
#include "entry.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <ctime>
#include <sys/prctl.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

using namespace sprintz;

namespace {

// RAII device buffer for the host-pointer wrappers
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
};

// Host framing walk: how many bytes does this stream span and how many
// elements does it decode to?  Needed because the reference's decompress()
// signature carries no length (sprintz.h:20) but an H2D copy must be sized.
// Touches headers and run lengths only -- no sample is decoded here.
//
// The walk trusts nothing it reads: it stops with `false` as soon as the framing claims more than
// one call may carry -- kMaxCallElems decoded elements or kMaxCallBytes of stream -- so a garbage
// group count or run length cannot send it (or the H2D copy sized from it) across the address
// space.  (The reference has no such limit: it reads wherever its header points.)
constexpr uint64_t kMaxCallElems = 1ull << 31;
constexpr uint64_t kMaxCallBytes = 1ull << 32;
bool walk_stream(const uint8_t* s, int esz, int D, uint32_t ngroups, uint32_t remaining, bool lowdim,
                 uint64_t* nbytes, uint64_t* nelems, bool norle = false)
{
    const int W = 8 * esz, HB = esz == 1 ? 3 : 4;
    const uint32_t hdr_bytes = (2u * D * HB + 7u) / 8u;
    uint64_t pos = 0, blocks = 0;
    auto field = [&](const uint8_t* h, uint32_t idx) {
        const uint32_t bit = idx * HB;
        uint32_t x = h[bit >> 3];
        if (((bit & 7) + HB) > 8) x |= (uint32_t)h[(bit >> 3) + 1] << 8;
        return (x >> (bit & 7)) & ((1u << HB) - 1);
    };
    for (uint32_t g = 0; g < ngroups; g++) {
        if (pos > kMaxCallBytes || blocks * 8ull * D > kMaxCallElems) return false;
        const uint8_t* h = s + pos;
        pos += hdr_bytes;
        for (int slot = 0; slot < 2; slot++) {
            uint32_t total = 0;
            for (int d = 0; d < D; d++) {
                uint32_t f = field(h, slot * D + d);
                total += (f == (uint32_t)(W - 1)) ? (uint32_t)W : f;
            }
            if (total == 0 && norle) {
                blocks += 1;                                   // a block of zeros has no payload
            } else if (total == 0) {
                uint32_t b0 = s[pos++], len = b0 & 0x7f;
                if (b0 & 0x80) len |= (uint32_t)s[pos++] << 7;
                blocks += len;
            } else {
                pos += lowdim ? total : 8ull * ((total + 7) / 8);
                blocks += 1;
            }
        }
    }
    *nbytes = pos + (uint64_t)remaining * esz;
    *nelems = blocks * 8ull * D + remaining;
    return *nbytes <= kMaxCallBytes && *nelems <= kMaxCallElems;
}

// ---- per-thread scratch of the host-pointer entry points -------------------------------------
// lzbench drives the single-call symbols once per 10 KB block, so they must not pay for
// hipMalloc/hipFree and pageable copies on every call: each thread keeps ONE device buffer and
// ONE pinned staging buffer that only grow, and a private non-blocking stream.  A call is then
// memcpy -> one H2D -> kernel -> one D2H -> memcpy, one stream synchronisation.  A thread that
// ends hands its scratch to a process-wide free list (no HIP call runs in a thread_local
// destructor; nothing is freed before the process ends).
struct Scratch {
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t* dev = nullptr;
    size_t dev_cap = 0;
    uint8_t* pin = nullptr;              // hipHostMallocMapped | Coherent: the kernels of a single call read and write it directly
    uint8_t* pin_dev = nullptr;          // the same bytes as the device sees them (hipHostGetDevicePointer)
    size_t pin_cap = 0;
    hipEvent_t done_spin = nullptr;      // waited for by spinning (a shared stream: the call waits for ITS launches, not for the stream)
    bool shared_stream = false;
    uint64_t* flag = nullptr;            // one mapped host word: the flag kernel that ends a polled call writes the call's ticket here
    uint64_t* flag_dev = nullptr;
    uint64_t ticket = 0;
    uint64_t last_wait_ns = 0;           // how long the last polled call of this thread waited
};
constexpr size_t kPinMax = 4u << 20;     // larger transfers go straight from/to the caller's memory

// ---- waiting for a single call's launches ---------------------------------------------------------
// hipStreamSynchronize spins: the shortest wait there is while the waiting threads have cores to spin on.  With more
// callers inside the library than that (lzbench -T64 in a 16-CPU container: 64 spinners on 16 CPUs' worth of quota get
// throttled, and the one whose kernel HAS finished waits for a time slice) a call ends with a kernel that writes the call's
// ticket into a mapped host word, and the caller sleeps and polls that word instead (a blocking-sync event was no better
// than spinning: the runtime's wait is where the CPU time went).  SPRINTZ_OPT_HOST_WAIT: 0 = by the number of callers (default), 1 = always spin, 2 = always sleep.
std::atomic<int> g_calls_inside{0};
int spin_budget()
{
    static const int n = [] {
        long q = (long)std::thread::hardware_concurrency();
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {           // cgroup v2 CPU quota, if any
            long quota = 0, period = 0;
            if (fscanf(f, "%ld %ld", &quota, &period) == 2 && quota > 0 && period > 0) q = std::min(q > 0 ? q : quota / period, quota / period);
            fclose(f);
        }
        return (int)std::min(4l, std::max(1l, q / 2));                   // half of them (the callers do other work too), and no more than 4: from 5
                                                                         // callers on the sleeping wait is the faster one (tools/mt_cmd.sh)
    }();
    return n;
}
struct CallGuard {
    int n;
    CallGuard() : n(g_calls_inside.fetch_add(1, std::memory_order_relaxed) + 1) {}
    ~CallGuard() { g_calls_inside.fetch_sub(1, std::memory_order_relaxed); }
};

std::mutex g_scratch_mu;
std::vector<Scratch*> g_scratch_free;
std::map<int, std::vector<hipStream_t>> g_stream_pool;      // per device: the streams the host-pointer calls share
std::map<int, size_t> g_stream_next;

struct ScratchHolder {
    Scratch* s = nullptr;
    ~ScratchHolder()
    {
        if (!s) return;
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        g_scratch_free.push_back(s);
    }
};
thread_local ScratchHolder t_scratch;

size_t round_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }

// this thread's scratch on the current device, with at least dev_bytes / pin_bytes of room
int acquire_scratch(size_t dev_bytes, size_t pin_bytes, Scratch** out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    Scratch* sc = t_scratch.s;
    if (sc && sc->device != dev) {                       // the thread moved to another device
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        g_scratch_free.push_back(sc);
        sc = t_scratch.s = nullptr;
    }
    if (!sc) {
        {
            std::lock_guard<std::mutex> lk(g_scratch_mu);
            for (size_t i = 0; i < g_scratch_free.size(); i++)
                if (g_scratch_free[i]->device == dev) {
                    sc = g_scratch_free[i];
                    g_scratch_free.erase(g_scratch_free.begin() + (long)i);
                    break;
                }
        }
        if (!sc) {
            sc = new Scratch();
            sc->device = dev;
            // The threads of a process share a FEW streams (SPRINTZ_OPT_HOST_STREAMS, default 4 = the hardware queues the runtime
            // maps streams onto): with a private stream per thread, 64 callers made 64 streams that the runtime multiplexes over
            // its 4 queues with a barrier packet at every switch -- 64 threads got a third of the calls per second of 8.
            const int k = sprintz_mi355x_get_option(SPRINTZ_OPT_HOST_STREAMS);
            hipError_t e = hipSuccess;
            if (k > 0) {
                std::lock_guard<std::mutex> lk(g_scratch_mu);
                auto& pool = g_stream_pool[dev];
                if ((int)pool.size() < k) {
                    hipStream_t st = nullptr;
                    e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
                    if (e == hipSuccess) pool.push_back(st);
                }
                if (e == hipSuccess) { sc->stream = pool[g_stream_next[dev]++ % pool.size()]; sc->shared_stream = true; }
            } else {
                e = hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking);
            }
            if (e != hipSuccess) { delete sc; return fail(SPRINTZ_E_HIP, "hipStreamCreateWithFlags", e); }
            const char* what = "hipEventCreateWithFlags";
            e = hipEventCreateWithFlags(&sc->done_spin, hipEventDisableTiming);
            if (e != hipSuccess) sc->done_spin = nullptr;
            if (e == hipSuccess) { what = "hipHostMalloc (completion flag)"; e = hipHostMalloc((void**)&sc->flag, 64, hipHostMallocMapped | hipHostMallocCoherent); if (e != hipSuccess) sc->flag = nullptr; }
            if (e == hipSuccess) { *sc->flag = 0; what = "hipHostGetDevicePointer (completion flag)"; e = hipHostGetDevicePointer((void**)&sc->flag_dev, sc->flag, 0); }
            if (e != hipSuccess) {
                if (sc->flag) (void)hipHostFree(sc->flag);
                if (sc->done_spin) (void)hipEventDestroy(sc->done_spin);
                if (!sc->shared_stream) (void)hipStreamDestroy(sc->stream);
                delete sc;
                return fail(SPRINTZ_E_HIP, what, e);
            }
        }
        t_scratch.s = sc;
    }
    if (sc->dev_cap < dev_bytes) {
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if (sc->dev) (void)hipFree(sc->dev);
        sc->dev = nullptr; sc->dev_cap = 0;
        const size_t want = round_up(dev_bytes + dev_bytes / 2, 1u << 16);
        HIP_TRY(hipMalloc((void**)&sc->dev, want));
        sc->dev_cap = want;
    }
    if (sc->pin_cap < pin_bytes) {
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if (sc->pin) (void)hipHostFree(sc->pin);
        sc->pin = nullptr; sc->pin_cap = 0;
        const size_t want = round_up(pin_bytes + pin_bytes / 2, 1u << 16);
        HIP_TRY(hipHostMalloc((void**)&sc->pin, want, hipHostMallocMapped | hipHostMallocCoherent));
        sc->pin_cap = want;
        HIP_TRY(hipHostGetDevicePointer((void**)&sc->pin_dev, sc->pin, 0));
    }
    *out = sc;
    return 0;
}

// ends a polled call: one word, the call's ticket, into the thread's mapped flag (after the codec kernel in stream order; a kernel's
// end makes its stores to host memory visible before the next kernel of the stream starts)
__global__ void flag_kernel(uint64_t* flag, uint64_t ticket)
{
    __hip_atomic_store(flag, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// sleep, then look at the thread's flag word until it holds `want`: no runtime wait at all (tools/mt_cmd.sh, 16-CPU container:
// 64 threads 200k calls/s this way, 48k on a blocking-sync event, 52k spinning).  spin: look without sleeping (few callers).
int wait_flag(Scratch* sc, uint64_t want, bool spin)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (spin) {
        for (uint32_t it = 1;; ++it) {
            if (__atomic_load_n(sc->flag, __ATOMIC_ACQUIRE) == want) break;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            if ((it & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                HIP_TRY(hipStreamSynchronize(sc->stream));               // a fault surfaces here
                if (__atomic_load_n(sc->flag, __ATOMIC_ACQUIRE) != want) return fail(SPRINTZ_E_HIP, "the call's completion flag was never written");
                break;
            }
        }
    } else {
        // the default 50 us of timer slack would make every 20 us sleep a 75 us one: 1 us for the duration of THIS wait, the caller's
        // own value put back before returning (it is the application's thread, not ours)
        struct SlackGuard {
            long old;
            SlackGuard() : old(prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0)) { if (old > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000ul, 0, 0, 0); }
            ~SlackGuard() { if (old > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old, 0, 0, 0); }
        } slack_guard;
        // first sleep: three quarters of what the thread's last call waited (with many callers a call queues behind the others' for
        // hundreds of microseconds), never under 15 us (no call is shorter); then 5, 10, 20 ... 160 us: 128 threads that each woke
        // every 5 us would spend the container's CPUs on waking up
        struct timespec ts{0, (long)std::min<uint64_t>(std::max<uint64_t>(15000, sc->last_wait_ns * 3 / 4), 2000000)};
        long step = 5000;
        for (uint32_t it = 0;; ++it) {
            nanosleep(&ts, nullptr);
            if (__atomic_load_n(sc->flag, __ATOMIC_ACQUIRE) == want) break;
            ts.tv_nsec = step;
            step = std::min(step * 2, 160000l);
            if ((it & 15) == 15 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                HIP_TRY(hipStreamSynchronize(sc->stream));
                if (__atomic_load_n(sc->flag, __ATOMIC_ACQUIRE) != want) return fail(SPRINTZ_E_HIP, "the call's completion flag was never written");
                break;
            }
        }
        sc->last_wait_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    if ((want & 63) == 0) (void)hipStreamQuery(sc->stream);          // the runtime retires finished launches when asked about them
    return 0;
}

bool spin_wait(int callers)
{
    const int mode = sprintz_mi355x_get_option(SPRINTZ_OPT_HOST_WAIT);
    return mode == 1 || (mode == 0 && callers <= spin_budget());
}

// wait for everything this call put on the thread's stream
int wait_call(Scratch* sc, int callers)
{
    if (spin_wait(callers)) {
        if (sc->shared_stream) {
            HIP_TRY(hipEventRecord(sc->done_spin, sc->stream));
            HIP_TRY(hipEventSynchronize(sc->done_spin));
        } else {
            HIP_TRY(hipStreamSynchronize(sc->stream));
        }
        return 0;
    }
    const uint64_t want = ++sc->ticket;
    hipLaunchKernelGGL(flag_kernel, dim3(1), dim3(1), 0, sc->stream, sc->flag_dev, want);
    HIP_TRY(hipGetLastError());
    return wait_flag(sc, want, false);
}

// A single call's input, host -> HBM, as ONE wide read of the thread's mapped staging buffer (every lane a 16-byte piece,
// all requests of the call in flight over PCIe at once): the codec kernels walk their streams in dependent steps, which
// must find them in HBM/L2 -- a PCIe round trip per step would cost more than the whole call.  Launched on the call's
// stream right before the codec kernel; n16 = 16-byte pieces.
typedef uint32_t stage_v4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) stage_in_kernel(const stage_v4* __restrict__ host, stage_v4* __restrict__ dev, uint32_t n16)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u)
        dev[i] = __builtin_nontemporal_load(host + i);
}
int stage_in(Scratch* sc, size_t pin_off, size_t dev_off, size_t bytes)
{
    const uint32_t n16 = (uint32_t)((bytes + 15) / 16);
    const unsigned grid = std::min<unsigned>((n16 + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(stage_in_kernel, dim3(grid), dim3(256), 0, sc->stream, (const stage_v4*)(sc->pin_dev + pin_off), (stage_v4*)(sc->dev + dev_off), n16);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what an encoder reported at `meta`: [size (u32) | . | ret (i64)]
int read_encoded(const uint8_t* meta, size_t bound, uint32_t* size, int64_t* ret)
{
    memcpy(size, meta, 4);
    memcpy(ret, meta + 8, 8);
    return *size > bound ? fail(SPRINTZ_E_HIP, "encoder reported a size above its bound") : 0;
}
// ... and a decoder: the elements it wrote, at most nelems, or its refusal
int read_decoded(const uint8_t* at, uint64_t nelems, int64_t* ret)
{
    memcpy(ret, at, 8);
    if (*ret < 0) return fail((int)*ret, "decoder rejected the stream");
    return (uint64_t)*ret > nelems ? fail(SPRINTZ_E_CORRUPT, "decoder rejected the stream") : 0;
}

int64_t compress_host(int codec, int esz, const void* src, uint32_t len, void* dest, uint16_t ndims, int write_size,
                      int layout = SPRINTZ_LAYOUT_AUTO)
{
    if (ndims == 0) { fail(SPRINTZ_E_INVALID, "ndims == 0"); return -1; }          // sprintz.cpp:36
    int rc = check_common(codec, esz, ndims);
    if (rc) return rc;
    if (layout < SPRINTZ_LAYOUT_AUTO || layout > SPRINTZ_LAYOUT_LOWDIM || (layout && codec > SPRINTZ_CODEC_XFF))
        return fail(SPRINTZ_E_INVALID, "layout must be 0 (by ndims), 1 (general) or 2 (low-dim), RLE codecs only");
    if (layout == SPRINTZ_LAYOUT_LOWDIM && !is_lowdim(esz, ndims)) {               // sprintz_delta_lowdim.cpp:64-70
        fail(SPRINTZ_E_INVALID, "the low-dim layout takes ndims <= 4 at 8 bits, <= 2 at 16 bits");
        return -1;
    }
    if (len > (1u << 30)) return fail(SPRINTZ_E_UNSUPPORTED, "single call limited to 2^30 elements");
    if ((rc = ensure_device())) return rc;
    if (len == 0 && codec == SPRINTZ_CODEC_XFF_NORLE) {     // u64 0 with ndims in bytes 6..7 (sprintz_xff.cpp:58-63)
        uint8_t h[8] = {0, 0, 0, 0, 0, 0, (uint8_t)(ndims & 0xff), (uint8_t)(ndims >> 8)};
        memcpy(dest, h, 8);
        return 8;
    }
    if (len == 0 && codec >= SPRINTZ_CODEC_DELTA_NORLE) {   // {u32 0; u16 ndims} (format.h:65-72)
        uint8_t h[6] = {0, 0, 0, 0, (uint8_t)(ndims & 0xff), (uint8_t)(ndims >> 8)};
        memcpy(dest, h, 6);
        return 6 / esz;
    }
    if (len == 0) {   // zero elements: header only (reference: :116-124 with len == 0)
        uint8_t h[8] = {0};
        h[6] = (uint8_t)(ndims & 0xff); h[7] = (uint8_t)(ndims >> 8);
        if (write_size) memcpy(dest, h, 8);
        return write_size ? 8 / esz : 0;
    }
    const size_t bound = sprintz_mi355x_compress_bound(esz, len, ndims);
    const size_t src_bytes = (size_t)len * esz;
    CallGuard inside;
    const Knobs knobs = snapshot();
    const int general = layout == SPRINTZ_LAYOUT_GENERAL;
    // ---- the zero-copy call (everything that fits the staging buffer; the RLE codecs, whose encoders only WRITE their slot):
    // memcpy into the mapped staging buffer -> stage_in + encoder on the thread's stream, the encoder's slot, size and return
    // value landing straight in the staging buffer -> ONE wait -> memcpy out.  No copy engine, no memset, no second round trip.
    // staging: [source | size, ret (16 B) | slot]      device: [source + read slack]
    if (codec <= SPRINTZ_CODEC_XFF && ndims <= 2047 && src_bytes + 16 + bound + 512 <= kPinMax) {      // (above 2047 columns the encoder ORs into its slot with device atomics: a slot in HBM)
        const size_t p_meta = round_up(src_bytes + 16, 256), p_slot = p_meta + 16;
        Scratch* sc = nullptr;
        if ((rc = acquire_scratch(round_up(src_bytes, 16) + SPRINTZ_MI355X_READ_SLACK, p_slot + bound, &sc))) return rc;
        memcpy(sc->pin, src, src_bytes);
        uint32_t size = 0xffffffffu;         // a kernel that never reports must read as an error, not as the last call's answer
        int64_t ret = -1;
        memcpy(sc->pin + p_meta, &size, 4);
        memcpy(sc->pin + p_meta + 8, &ret, 8);
        // one chunk the workgroup-per-chunk encoder takes: it reads the staging buffer itself (one wide read, as stage_in's) and
        // ends the call by writing the ticket -- ONE launch, no runtime wait.  Planned ONCE, for the staging addresses: the plan that
        // chooses the ticket form is the plan the launcher runs
        EncodeBatch j{codec, esz, sc->pin_dev, len, len, ndims, sc->pin_dev + p_slot, bound, (uint32_t*)(sc->pin_dev + p_meta), (int64_t*)(sc->pin_dev + p_meta + 8), write_size, 0, general};
        const Plan zc = plan_encode(encode_shape(j, false, true), knobs);
        if (zc.family == SPRINTZ_KF_ENC_LAT) {
            HostCall hc;
            hc.flag = sc->flag_dev;
            hc.ticket = ++sc->ticket;
            if ((rc = encode_launch(zc, j, sc->stream, nullptr, &hc))) return rc;
            if ((rc = wait_flag(sc, hc.ticket, spin_wait(inside.n)))) { (void)hipStreamSynchronize(sc->stream); *sc->flag = 0; return rc; }   // nothing of this call may still target sc->pin / sc->flag when the scratch is reused
        } else {
            if ((rc = stage_in(sc, 0, 0, src_bytes))) return rc;
            j.src = sc->dev;
            if ((rc = encode_batch(knobs, j, sc->stream))) { (void)hipStreamSynchronize(sc->stream); return rc; }   // stage_in may still be reading sc->pin
            if ((rc = wait_call(sc, inside.n))) return rc;
        }
        if ((rc = read_encoded(sc->pin + p_meta, bound, &size, &ret))) return rc;
        memcpy(dest, sc->pin + p_slot, size);
        return ret;
    }
    // ---- larger calls and the run-less codecs -- device scratch: [source + read slack | size, ret (16 B) | slot]
    const size_t o_meta = round_up(src_bytes + SPRINTZ_MI355X_READ_SLACK, 256), o_slot = o_meta + 16;
    const bool pin_in = src_bytes <= kPinMax, pin_out = 16 + bound <= kPinMax;
    Scratch* sc = nullptr;
    if ((rc = acquire_scratch(o_slot + bound, std::max(pin_in ? src_bytes : 0, pin_out ? 16 + bound : 0), &sc))) return rc;
    if (pin_in) memcpy(sc->pin, src, src_bytes);
    HIP_TRY(hipMemcpyAsync(sc->dev, pin_in ? sc->pin : src, src_bytes, hipMemcpyHostToDevice, sc->stream));
    uint32_t* d_size = (uint32_t*)(sc->dev + o_meta);
    int64_t* d_ret = (int64_t*)(sc->dev + o_meta + 8);
    // the scratch is reused: a kernel that never reports must read as an error (size 0xffffffff > bound), not as the last call's answer
    HIP_TRY(hipMemsetAsync(d_size, 0xff, 16, sc->stream));
    rc = encode_batch(knobs, EncodeBatch{codec, esz, sc->dev, len, len, ndims, sc->dev + o_slot, bound, d_size, d_ret, write_size, 0, general}, sc->stream);
    if (rc) { (void)hipStreamSynchronize(sc->stream); return rc; }   // the H2D copy out of sc->pin may still be in flight
    uint32_t size = 0;
    int64_t ret = 0;
    // small slots: size, ret and the whole slot in one copy (one round trip); large ones: the 16 bytes first, then exactly `size`
    // bytes -- a compressible multi-megabyte call would otherwise move 2-4x the stream over PCIe
    constexpr size_t kOneCopyMax = 64u << 10;
    if (pin_out && 16 + bound <= kOneCopyMax) {
        HIP_TRY(hipMemcpyAsync(sc->pin, sc->dev + o_meta, 16 + bound, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if ((rc = read_encoded(sc->pin, bound, &size, &ret))) return rc;
        memcpy(dest, sc->pin + 16, size);
    } else {                                                   // through the staging buffer where the slot fits it, else straight to the caller's memory
        uint8_t meta[16];
        uint8_t* const m = pin_out ? sc->pin : meta;
        HIP_TRY(hipMemcpyAsync(m, sc->dev + o_meta, 16, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if ((rc = read_encoded(m, bound, &size, &ret))) return rc;
        HIP_TRY(hipMemcpyAsync(pin_out ? (void*)sc->pin : dest, sc->dev + o_slot, size, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if (pin_out) memcpy(dest, sc->pin, size);
    }
    return ret;
}

// shared tail of the single-call decoders: stream [s, s + nbytes) (host) -> nelems elements.
// device scratch: [offsets[2] (16 B) | stream + read slack | ret (16 B) | out]
// plain: a decode in the layout its ndims implies and nothing else -- `spec` carries its framing alone
int64_t decode_host_common(int codec, int esz, const uint8_t* s, uint64_t nbytes, uint64_t nelems, uint16_t ndims, void* dest,
                           bool plain, const QuerySpec& spec, uint64_t* result)
{
    const size_t o_out_meta = round_up(16 + nbytes + SPRINTZ_MI355X_READ_SLACK, 256), o_out = o_out_meta + 16;
    const size_t out_bytes = (size_t)nelems * esz;
    const bool want_out = spec.q != kQueryReduceOnly;
    Batch b{codec, esz, nullptr, nullptr, 1, (uint32_t)nelems, ndims};      // one chunk: the stream, where the call puts it
    CallGuard inside;
    const Knobs knobs = snapshot();
    // ---- the zero-copy call (plain decodes that fit the staging buffer): memcpy the stream into the mapped staging buffer ->
    // stage_in + decoder on the thread's stream, the decoder writing samples and its return value straight into the staging
    // buffer -> ONE wait -> memcpy out.   staging: [offsets[2] | stream | ret (16 B) | out]      device: [offsets[2] | stream + slack]
    if (plain && ndims <= 2047 && 16 + nbytes + 512 + 16 + out_bytes <= kPinMax) {      // (above 2047 columns the decoder reads its own output back: an output in HBM)
        const size_t p_ret = round_up(16 + nbytes + 16, 256), p_out = p_ret + 16;
        Scratch* sc = nullptr;
        int rc = acquire_scratch(round_up(16 + nbytes, 16) + SPRINTZ_MI355X_READ_SLACK, p_out + out_bytes, &sc);
        if (rc) return rc;
        const uint64_t meta[2] = {16, 16 + nbytes};
        int64_t ret = -1;
        memcpy(sc->pin, meta, 16);
        memcpy(sc->pin + 16, s, nbytes);
        memcpy(sc->pin + p_ret, &ret, 8);
        HostCall hc;
        hc.off0 = 16; hc.off1 = 16 + nbytes;
        hc.flag = sc->flag_dev;
        QuerySpec qs = spec;
        qs.hc = &hc;
        b.comp = sc->pin_dev;
        const Plan zc = plan_decode(decode_shape(b, sc->pin_dev + p_out, qs), knobs);   // (see compress_host)
        if (zc.family == SPRINTZ_KF_DEC_LAT) {
            hc.ticket = ++sc->ticket;
            if ((rc = decode_launch(zc, b, sc->pin_dev + p_out, (int64_t*)(sc->pin_dev + p_ret), sc->stream, qs))) return rc;
            if ((rc = wait_flag(sc, hc.ticket, spin_wait(inside.n)))) { (void)hipStreamSynchronize(sc->stream); *sc->flag = 0; return rc; }   // nothing of this call may still target sc->pin / sc->flag when the scratch is reused
        } else {
            if ((rc = stage_in(sc, 0, 0, 16 + nbytes))) return rc;
            b.comp = sc->dev;
            b.offsets = (const uint64_t*)sc->dev;
            rc = decode_batch(knobs, b, sc->pin_dev + p_out, (int64_t*)(sc->pin_dev + p_ret), sc->stream, spec);
            if (rc) { (void)hipStreamSynchronize(sc->stream); return rc; }
            if ((rc = wait_call(sc, inside.n))) return rc;
        }
        if ((rc = read_decoded(sc->pin + p_ret, nelems, &ret))) return rc;
        memcpy(dest, sc->pin + p_out, (size_t)ret * esz);
        return ret;
    }
    const size_t o_res = round_up(o_out + (want_out ? out_bytes : 0), 256);
    const size_t res_bytes = spec.qop ? (size_t)ndims * 8 : 0;
    const bool pin_in = 16 + nbytes <= kPinMax, pin_out = 16 + out_bytes <= kPinMax;
    Scratch* sc = nullptr;
    int rc = acquire_scratch(o_res + res_bytes, std::max<size_t>(std::max<size_t>(pin_in ? 16 + nbytes : 16, pin_out ? 16 + out_bytes : 16), res_bytes), &sc);
    if (rc) return rc;
    const uint64_t meta[2] = {16, 16 + nbytes};              // offsets[0], offsets[1] (= stream end) relative to the scratch
    memcpy(sc->pin, meta, 16);
    if (pin_in) memcpy(sc->pin + 16, s, nbytes);
    HIP_TRY(hipMemcpyAsync(sc->dev, sc->pin, pin_in ? 16 + nbytes : 16, hipMemcpyHostToDevice, sc->stream));
    if (!pin_in) HIP_TRY(hipMemcpyAsync(sc->dev + 16, s, nbytes, hipMemcpyHostToDevice, sc->stream));
    int64_t* d_ret = (int64_t*)(sc->dev + o_out_meta);
    HIP_TRY(hipMemsetAsync(d_ret, 0xff, 8, sc->stream));      // a kernel that never reports reads as an error
    QuerySpec qs = spec;
    if (res_bytes) {
        qs.qres = (uint64_t*)(sc->dev + o_res);
        HIP_TRY(hipMemsetAsync(qs.qres, 0, res_bytes, sc->stream));
    }
    b.comp = sc->dev;
    b.offsets = (const uint64_t*)sc->dev;
    rc = decode_batch(knobs, b, want_out ? sc->dev + o_out : nullptr, d_ret, sc->stream, qs);
    if (rc) { (void)hipStreamSynchronize(sc->stream); return rc; }   // the H2D copy out of sc->pin may still be in flight
    int64_t ret = 0;
    if (want_out && pin_out) {                                // ret and the samples in one copy
        HIP_TRY(hipMemcpyAsync(sc->pin, sc->dev + o_out_meta, 16 + out_bytes, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if ((rc = read_decoded(sc->pin, nelems, &ret))) return rc;
        memcpy(dest, sc->pin + 16, (size_t)ret * esz);
    } else {
        HIP_TRY(hipMemcpyAsync(sc->pin, d_ret, 8, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if ((rc = read_decoded(sc->pin, nelems, &ret))) return rc;
        if (want_out) {
            HIP_TRY(hipMemcpyAsync(dest, sc->dev + o_out, (size_t)ret * esz, hipMemcpyDeviceToHost, sc->stream));
            HIP_TRY(hipStreamSynchronize(sc->stream));
        }
    }
    if (result && res_bytes) {
        HIP_TRY(hipMemcpyAsync(sc->pin, sc->dev + o_res, res_bytes, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        memcpy(result, sc->pin, res_bytes);
    }
    return ret;
}

// noheader: the framing comes with the call (sprintz_mi355x_decompress_noheader), not from the stream's first 8 bytes
int64_t decompress_host(int codec, int esz, const void* src, void* dest, int layout = SPRINTZ_LAYOUT_AUTO, int noheader = 0, uint16_t nh_ndims = 0,
                        uint32_t nh_ngroups = 0, uint16_t nh_remaining = 0)
{
    if (layout < SPRINTZ_LAYOUT_AUTO || layout > SPRINTZ_LAYOUT_LOWDIM || (layout && codec > SPRINTZ_CODEC_XFF))
        return fail(SPRINTZ_E_INVALID, "layout must be 0 (by ndims), 1 (general) or 2 (low-dim), RLE codecs only");
    const uint8_t* s = (const uint8_t*)src;
    uint32_t ngroups, remaining;
    uint16_t ndims;
    const bool norle = codec >= SPRINTZ_CODEC_DELTA_NORLE;
    if (norle) {                                               // {u32 len; u16 ndims}; sprintz_delta.cpp:803-807, :832
        uint32_t len;
        memcpy(&len, s, 4);
        memcpy(&ndims, s + (codec == SPRINTZ_CODEC_XFF_NORLE ? 6 : 4), 2);
        ngroups = (len < 128 || ndims == 0) ? 0 : len / (16u * ndims);
        remaining = len - ngroups * 16u * ndims;
        if (ndims == 0 && len == 0) return 0;
    } else if (!noheader) {
        uint16_t r16;
        memcpy(&ngroups, s, 4);
        memcpy(&r16, s + 4, 2);
        memcpy(&ndims, s + 6, 2);
        remaining = r16;
    } else {
        ngroups = nh_ngroups; remaining = nh_remaining; ndims = nh_ndims;
    }
    if (ndims == 0) { fail(SPRINTZ_E_INVALID, "ndims == 0"); return -1; }          // sprintz.cpp:36
    int rc = check_common(codec, esz, ndims);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    if (layout == SPRINTZ_LAYOUT_LOWDIM && !is_lowdim(esz, ndims)) {               // sprintz_delta_lowdim.cpp:423-429
        fail(SPRINTZ_E_INVALID, "the low-dim layout takes ndims <= 4 at 8 bits, <= 2 at 16 bits");
        return -1;
    }
    const bool general = layout == SPRINTZ_LAYOUT_GENERAL;
    const uint32_t hlen = norle ? (codec == SPRINTZ_CODEC_XFF_NORLE ? 8 : 6) : (noheader ? 0 : 8);
    uint64_t nbytes = 0, nelems = 0;
    if (!walk_stream(s + hlen, esz, ndims, ngroups, remaining, (norle || general) ? false : is_lowdim(esz, ndims), &nbytes, &nelems, norle))
        return fail(SPRINTZ_E_UNSUPPORTED, "stream framing exceeds the single-call limits (2^31 elements / 4 GiB): damaged header?");
    nbytes += hlen;
    if (nelems == 0) return 0;
    QuerySpec qs;
    qs.general = general ? 1 : 0;
    qs.noheader = noheader; qs.nh_ngroups = ngroups; qs.nh_remaining = remaining;
    return decode_host_common(codec, esz, s, nbytes, nelems, ndims, dest, !general, qs, nullptr);
}

// single-call query (mirrors query_rowmajor_{delta,xff}_rle_{8b,16b}: sprintz_delta.h:95-98,
// sprintz_xff.h:90-93): host stream in, optional materialised data and per-column result out
int64_t query_host(int codec, int esz, const void* src, void* dest, int op, int materialize, uint64_t* result, uint32_t flags)
{
    const int general = (flags & SPRINTZ_QUERY_GENERAL_LAYOUT) != 0;
    if (op < 0 || op > 2) return fail(SPRINTZ_E_INVALID, "op must be 0 (none), 1 (max) or 2 (sum)");
    if (materialize && !dest) return fail(SPRINTZ_E_INVALID, "materialize without a destination");
    const uint8_t* s = (const uint8_t*)src;
    uint32_t ngroups;
    uint16_t r16, ndims;
    memcpy(&ngroups, s, 4);
    memcpy(&r16, s + 4, 2);
    memcpy(&ndims, s + 6, 2);
    const uint32_t remaining = r16;
    if (ndims == 0) { fail(SPRINTZ_E_INVALID, "ndims == 0"); return -1; }
    int rc = check_common(codec, esz, ndims);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    uint64_t nbytes = 0, nelems = 0;
    if (!walk_stream(s + 8, esz, ndims, ngroups, remaining, general ? false : is_lowdim(esz, ndims), &nbytes, &nelems))
        return fail(SPRINTZ_E_UNSUPPORTED, "stream framing exceeds the single-call limits (2^31 elements / 4 GiB): damaged header?");
    nbytes += 8;
    if (result) memset(result, 0, (size_t)ndims * 8);
    if (nelems == 0) return 0;
    QuerySpec qs;
    qs.q = materialize ? (op ? kQueryMaterialize : kQueryOff) : kQueryReduceOnly;
    qs.qop = op;
    qs.general = general;
    return decode_host_common(codec, esz, s, nbytes, nelems, ndims, dest, false, qs, result);
}

}  // namespace

// what the other translation units' host-pointer entry points (online.hip) share with this one: the calling thread's pooled
// scratch (one device buffer, one pinned buffer, one non-blocking stream)
int sprintz::host_scratch(size_t dev_bytes, size_t pin_bytes, HostScratch* out)
{
    Scratch* sc = nullptr;
    const int rc = acquire_scratch(dev_bytes, pin_bytes, &sc);
    if (rc) return rc;
    *out = HostScratch{sc->stream, sc->dev, sc->pin};
    return 0;
}

extern "C" {

// ---- drop-in single-call API (host pointers)
int64_t sprintz_mi355x_compress_delta_8b(const uint8_t* s, uint32_t n, int8_t* d, uint16_t nd, int ws)    { return compress_host(SPRINTZ_CODEC_DELTA, 1, s, n, d, nd, ws); }
int64_t sprintz_mi355x_compress_xff_8b(const uint8_t* s, uint32_t n, int8_t* d, uint16_t nd, int ws)      { return compress_host(SPRINTZ_CODEC_XFF, 1, s, n, d, nd, ws); }
int64_t sprintz_mi355x_compress_delta_16b(const uint16_t* s, uint32_t n, int16_t* d, uint16_t nd, int ws) { return compress_host(SPRINTZ_CODEC_DELTA, 2, s, n, d, nd, ws); }
int64_t sprintz_mi355x_compress_xff_16b(const uint16_t* s, uint32_t n, int16_t* d, uint16_t nd, int ws)   { return compress_host(SPRINTZ_CODEC_XFF, 2, s, n, d, nd, ws); }

int64_t sprintz_mi355x_decompress_delta_8b(const int8_t* s, uint8_t* d)    { return decompress_host(SPRINTZ_CODEC_DELTA, 1, s, d); }
int64_t sprintz_mi355x_decompress_xff_8b(const int8_t* s, uint8_t* d)      { return decompress_host(SPRINTZ_CODEC_XFF, 1, s, d); }
int64_t sprintz_mi355x_decompress_delta_16b(const int16_t* s, uint16_t* d) { return decompress_host(SPRINTZ_CODEC_DELTA, 2, s, d); }
int64_t sprintz_mi355x_decompress_xff_16b(const int16_t* s, uint16_t* d)   { return decompress_host(SPRINTZ_CODEC_XFF, 2, s, d); }

int64_t sprintz_mi355x_decompress_noheader(int codec, int elem_bytes, const void* src, void* dest, uint16_t ndims,
                                           uint32_t ngroups, uint16_t remaining_len)
{
    return decompress_host(codec, elem_bytes, src, dest, SPRINTZ_LAYOUT_AUTO, 1, ndims, ngroups, remaining_len);
}

int64_t sprintz_mi355x_compress_layout(int codec, int elem_bytes, const void* src, uint32_t len, void* dest, uint16_t ndims,
                                       int write_size, int layout)
{
    return compress_host(codec, elem_bytes, src, len, dest, ndims, write_size, layout);
}

int64_t sprintz_mi355x_decompress_layout(int codec, int elem_bytes, const void* src, void* dest, int layout)
{
    return decompress_host(codec, elem_bytes, src, dest, layout);
}

// ---- host convenience: chunked codec over host buffers
int64_t sprintz_mi355x_compress_chunked_host(int codec, int elem_bytes, const void* src, uint64_t total_len, uint32_t chunk_len,
                                             uint16_t ndims, void* comp, size_t comp_capacity, uint64_t* offsets)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (chunk_len == 0) return fail(SPRINTZ_E_INVALID, "chunk_len == 0");
    if ((rc = check_batch_tail(total_len, chunk_len, ndims))) return rc;
    if ((rc = ensure_device())) return rc;
    const uint64_t nchunks = sprintz_mi355x_num_chunks(total_len, chunk_len);
    if (nchunks == 0) { offsets[0] = 0; return 0; }
    const size_t stride = sprintz_mi355x_compress_bound(elem_bytes, chunk_len, ndims);
    DevBuf d_src, d_slots, d_sizes, d_dense, d_offs, d_tmp;
    HIP_TRY(d_src.alloc(total_len * elem_bytes + SPRINTZ_MI355X_READ_SLACK));
    HIP_TRY(d_slots.alloc(stride * nchunks));
    HIP_TRY(d_sizes.alloc(nchunks * 4));
    HIP_TRY(d_offs.alloc((nchunks + 1) * 8));
    HIP_TRY(d_tmp.alloc(sprintz_mi355x_compact_tmp_bytes(nchunks)));
    HIP_TRY(d_dense.alloc(stride * nchunks + SPRINTZ_MI355X_READ_SLACK));
    HIP_TRY(hipMemcpy(d_src.p, src, total_len * elem_bytes, hipMemcpyHostToDevice));
    rc = encode_batch(snapshot(), EncodeBatch{codec, elem_bytes, d_src.p, total_len, chunk_len, ndims, d_slots.p, stride, (uint32_t*)d_sizes.p, nullptr}, nullptr);
    if (rc) return rc;
    rc = sprintz_mi355x_compact(d_slots.p, stride, (const uint32_t*)d_sizes.p, nchunks, 1, d_dense.p, (uint64_t*)d_offs.p,
                                d_tmp.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(offsets, d_offs.p, (nchunks + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t total = offsets[nchunks];
    if (total > comp_capacity) return fail(SPRINTZ_E_INVALID, "comp_capacity too small");
    HIP_TRY(hipMemcpy(comp, d_dense.p, total, hipMemcpyDeviceToHost));
    return (int64_t)total;
}

int64_t sprintz_mi355x_decompress_chunked_host(int codec, int elem_bytes, const void* comp, const uint64_t* offsets,
                                               uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, void* out)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (chunk_len == 0) return fail(SPRINTZ_E_INVALID, "chunk_len == 0");
    if ((rc = ensure_device())) return rc;
    if (nchunks == 0) return 0;
    const uint64_t total = offsets[nchunks];
    DevBuf d_comp, d_offs, d_out, d_rets;
    HIP_TRY(d_comp.alloc(total + SPRINTZ_MI355X_READ_SLACK));
    HIP_TRY(d_offs.alloc((nchunks + 1) * 8));
    HIP_TRY(d_out.alloc(nchunks * (uint64_t)chunk_len * elem_bytes));
    HIP_TRY(d_rets.alloc(nchunks * 8));
    HIP_TRY(hipMemcpy(d_comp.p, comp, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offs.p, offsets, (nchunks + 1) * 8, hipMemcpyHostToDevice));
    rc = decode_batch(Batch{codec, elem_bytes, d_comp.p, (const uint64_t*)d_offs.p, nchunks, chunk_len, ndims}, d_out.p, (int64_t*)d_rets.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<int64_t> rets(nchunks);
    HIP_TRY(hipMemcpy(rets.data(), d_rets.p, nchunks * 8, hipMemcpyDeviceToHost));
    int64_t sum = 0;
    for (uint64_t c = 0; c < nchunks; c++) {
        if (rets[c] < 0) return fail((int)rets[c], "decoder rejected a chunk stream");
        // the copy below takes `sum` CONTIGUOUS elements: every chunk but the last must be full
        if (c + 1 < nchunks && rets[c] != (int64_t)chunk_len)
            return fail(SPRINTZ_E_CORRUPT, "a chunk other than the last decoded to fewer than chunk_len elements");
        sum += rets[c];
    }
    // chunks are full except possibly the last: decoded data is contiguous
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)sum * elem_bytes, hipMemcpyDeviceToHost));
    return sum;
}

// ---- single-call queries (flags: SPRINTZ_QUERY_GENERAL_LAYOUT alone counts)
int64_t sprintz_mi355x_query_delta_8b(const int8_t* s, uint8_t* d, int op, int mat, uint32_t flags, uint64_t* res)    { return query_host(SPRINTZ_CODEC_DELTA, 1, s, d, op, mat, res, flags); }
int64_t sprintz_mi355x_query_delta_16b(const int16_t* s, uint16_t* d, int op, int mat, uint32_t flags, uint64_t* res) { return query_host(SPRINTZ_CODEC_DELTA, 2, s, d, op, mat, res, flags); }
int64_t sprintz_mi355x_query_xff_8b(const int8_t* s, uint8_t* d, int op, int mat, uint32_t flags, uint64_t* res)      { return query_host(SPRINTZ_CODEC_XFF, 1, s, d, op, mat, res, flags); }
int64_t sprintz_mi355x_query_xff_16b(const int16_t* s, uint16_t* d, int op, int mat, uint32_t flags, uint64_t* res)   { return query_host(SPRINTZ_CODEC_XFF, 2, s, d, op, mat, res, flags); }

// ---------------------------------------------------------------- non-RLE codecs, single call (host pointers)
int64_t sprintz_mi355x_compress_norle(int codec, int elem_bytes, const void* src, uint32_t len, void* dest, uint16_t ndims)
{
    if (codec < SPRINTZ_CODEC_DELTA_NORLE || codec > SPRINTZ_CODEC_XFF_NORLE) return fail(SPRINTZ_E_INVALID, "codec must be 2, 3 or 4");
    return compress_host(codec, elem_bytes, src, len, dest, ndims, 1);
}

int64_t sprintz_mi355x_decompress_norle(int codec, int elem_bytes, const void* src, void* dest)
{
    if (codec < SPRINTZ_CODEC_DELTA_NORLE || codec > SPRINTZ_CODEC_XFF_NORLE) return fail(SPRINTZ_E_INVALID, "codec must be 2, 3 or 4");
    return decompress_host(codec, elem_bytes, src, dest);
}

}  // extern "C"
