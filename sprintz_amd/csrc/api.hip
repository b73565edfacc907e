// api.hip -- the batched half of the C-ABI of libsprintz_mi355x.so (include/sprintz_mi355x.h) and what every entry unit
// stands on (entry.h): the process state, the error sink, the options, the launchers of what plan.h decided (which kernel,
// which geometry: no eligibility predicate lives here) and the size-scan / compaction kernels.  The single calls on host
// pointers are host_call.hip's, the row operations row_ops.hip's.  No codec arithmetic on the host.
#include "entry.h"

#include <atomic>
#include <climits>
#include <cstdlib>
#include <mutex>
#include <string>

#include "encode_blk.h"      // launch_encode_blk, launch_encode_blk_uni
#include "decode_blk.h"      // launch_decode_blk
#include "decode_row.h"      // launch_decode_row

using namespace sprintz;

namespace {

thread_local std::string g_last_error = "";

// Process-wide facts, established exactly once (the header promises re-entrancy from any thread):
// whether a HIP device exists at all, and the tuning knobs of the environment.
// (the knobs start from the environment, read once, and change only through sprintz_mi355x_set_option)
struct Process {
    bool have_device = false;
    std::atomic<int> no_fast{0};            // SPRINTZ_MI355X_NO_FAST: generic kernels only (A/B runs, tests)
    std::atomic<int> chunks_per_group{1};   // SPRINTZ_MI355X_CHUNKS_PER_GROUP (decode_fast read-ahead across chunks)
    std::atomic<int> dense_mode{1};         // SPRINTZ_MI355X_DENSE_MODE: how compress_batch_dense builds the container (see SPRINTZ_OPT_DENSE_MODE)
    std::atomic<int> enc_pair{1024};        // SPRINTZ_MI355X_ENC_PAIR: chunks from which row-major streams of 5 .. 64 columns are encoded with two columns per lane (0: never; see SPRINTZ_OPT_ENC_PAIR)
    std::atomic<int> blk_kernels{9};        // SPRINTZ_MI355X_BLK_KERNELS: which of round 6's delta kernels large batches take: bit 0 encode_blk (general layout), bit 1 decode_blk, bit 2 encode_blk_uni (univariate low-dim), bit 3 decode_row (wins over bit 1) on the shapes it wins on, bit 4 decode_row on every shape it fits
    std::atomic<int> blk_chunks{2049};      // SPRINTZ_MI355X_BLK_CHUNKS: batches of at least this many chunks take the block-parallel delta kernels (encode_blk.h; 0: never)
    std::atomic<int> lat_chunks{2048};      // SPRINTZ_MI355X_LAT_CHUNKS: batches of at most this many chunks decode with one workgroup per chunk (decode_lat.h; 0: never)
    std::atomic<int> ref_quirk{0};          // SPRINTZ_MI355X_REF_DECODER_QUIRK: decode as the reference DECODER does where it differs from the inverse of its encoder
    std::atomic<int> host_streams{4};       // SPRINTZ_MI355X_HOST_STREAMS: streams the host-pointer calls of all threads share per device (0: one per thread)
    std::atomic<int> host_wait{0};          // SPRINTZ_MI355X_HOST_WAIT: how a single call waits for its launches (see SPRINTZ_OPT_HOST_WAIT)
    std::atomic<int> split_lanes{1};        // SPRINTZ_MI355X_SPLIT_LANES: 8-bit streams of 65 .. 80 columns on 32 lanes x (pair + single) (see SPRINTZ_OPT_SPLIT_LANES)
};
Process& process()
{
    static Process p;
    static std::once_flag once;
    std::call_once(once, [] {
        int n = 0;
        p.have_device = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        p.no_fast = getenv("SPRINTZ_MI355X_NO_FAST") != nullptr ? 1 : 0;
        if (const char* e = getenv("SPRINTZ_MI355X_DENSE_MODE")) {
            const int k = atoi(e);
            p.dense_mode = k <= 0 ? 0 : 1;
        }
        if (const char* e = getenv("SPRINTZ_MI355X_LAT_CHUNKS")) p.lat_chunks = atoi(e) < 0 ? 0 : atoi(e);
        if (const char* e = getenv("SPRINTZ_MI355X_BLK_CHUNKS")) p.blk_chunks = atoi(e) < 0 ? 0 : atoi(e);
        if (const char* e = getenv("SPRINTZ_MI355X_BLK_KERNELS")) p.blk_kernels = atoi(e) & 31;
        if (const char* e = getenv("SPRINTZ_MI355X_REF_DECODER_QUIRK")) p.ref_quirk = atoi(e) != 0 ? 1 : 0;
        if (const char* e = getenv("SPRINTZ_MI355X_HOST_STREAMS")) p.host_streams = atoi(e) < 0 ? 0 : (atoi(e) > 64 ? 64 : atoi(e));
        if (const char* e = getenv("SPRINTZ_MI355X_HOST_WAIT")) p.host_wait = atoi(e) < 0 || atoi(e) > 2 ? 0 : atoi(e);
        if (const char* e = getenv("SPRINTZ_MI355X_SPLIT_LANES")) p.split_lanes = atoi(e) != 0 ? 1 : 0;
        if (const char* e = getenv("SPRINTZ_MI355X_ENC_PAIR")) p.enc_pair = atoi(e) < 0 ? 0 : atoi(e);
        if (const char* e = getenv("SPRINTZ_MI355X_CHUNKS_PER_GROUP")) {
            const int k = atoi(e);
            p.chunks_per_group = k < 1 ? 1 : k > 64 ? 64 : k;
        }
    });
    return p;
}

// The options that are a knob of Process: the values set_option takes for each and its refusal of any other (null: a flag -- every
// value is taken and stored as 0 / 1).  The two Huff0 options live in huf0.hip
struct Option { int id; std::atomic<int> Process::*knob; int lo, hi; const char* outside; };
const char* const kNotNegative = "the batch size must not be negative";
const Option kOptions[] = {
    {SPRINTZ_OPT_NO_FAST, &Process::no_fast, 0, 1, nullptr},
    {SPRINTZ_OPT_DENSE_MODE, &Process::dense_mode, 0, 1, "dense mode must be 0 or 1"},
    {SPRINTZ_OPT_SPLIT_LANES, &Process::split_lanes, 0, 1, nullptr},
    {SPRINTZ_OPT_ENC_PAIR, &Process::enc_pair, 0, INT_MAX, kNotNegative},
    {SPRINTZ_OPT_BLK_KERNELS, &Process::blk_kernels, 0, 31, "SPRINTZ_OPT_BLK_KERNELS is a mask of bits 0 .. 4"},
    {SPRINTZ_OPT_BLK_CHUNKS, &Process::blk_chunks, 0, 1 << 30, "SPRINTZ_OPT_BLK_CHUNKS must be in 0..2^30"},
    {SPRINTZ_OPT_LAT_CHUNKS, &Process::lat_chunks, 0, INT_MAX, kNotNegative},
    {SPRINTZ_OPT_REF_DECODER_QUIRK, &Process::ref_quirk, 0, 1, nullptr},
    {SPRINTZ_OPT_HOST_STREAMS, &Process::host_streams, 0, 64, "host streams must be in 0..64"},      // (threads that already hold a scratch keep their stream)
    {SPRINTZ_OPT_HOST_WAIT, &Process::host_wait, 0, 2, "host wait must be 0 (by callers), 1 (spin) or 2 (sleep)"},
    {SPRINTZ_OPT_CHUNKS_PER_GROUP, &Process::chunks_per_group, 1, 64, "chunks per group must be in 1..64"},
};
std::atomic<long long>* huf0_option(int option)
{
    return option == SPRINTZ_OPT_HUF0_BIG_BATCH ? &huf0_big_batch() : option == SPRINTZ_OPT_HUF0_SYNC_CHUNKS ? &huf0_sync_chunks() : nullptr;
}

// ---------------------------------------------------------------- compaction kernels

constexpr int kScanBlock = 1024;

__global__ void __launch_bounds__(kScanBlock) scan_local_kernel(const uint32_t* sizes, uint64_t n, uint32_t align,
                                                                uint64_t* offsets, uint64_t* block_sums)
{
    __shared__ uint64_t sh[kScanBlock];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint64_t a = align - 1;
    uint64_t v = i < n ? (((uint64_t)sizes[i] + a) & ~a) : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        uint64_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    if (i < n) offsets[i] = sh[threadIdx.x] - v;
    if (threadIdx.x == kScanBlock - 1) block_sums[blockIdx.x] = sh[threadIdx.x];
}

__global__ void __launch_bounds__(kScanBlock) scan_blocks_kernel(uint64_t* block_sums, uint64_t nblocks, uint64_t* total_out)
{
    __shared__ uint64_t sh[kScanBlock];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < nblocks; base += kScanBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nblocks ? block_sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kScanBlock; off <<= 1) {
            uint64_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblocks) block_sums[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) carry += sh[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(kScanBlock) scan_add_kernel(uint64_t* offsets, uint64_t n, const uint64_t* block_sums)
{
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    if (i < n) offsets[i] += block_sums[blockIdx.x];
}

// batches of up to kScanOne chunks: the whole scan in ONE workgroup (a thread takes kScanPer consecutive sizes, the 1 024 partial
// sums are scanned in LDS) -- one launch instead of three where the launches are what the scan costs (BASELINE config 5: 6 554 chunks)
constexpr int kScanPer = 16, kScanOne = kScanBlock * kScanPer;
__global__ void __launch_bounds__(kScanBlock) scan_one_kernel(const uint32_t* sizes, uint64_t n, uint32_t align, uint64_t* offsets)
{
    __shared__ uint64_t sh[kScanBlock];
    const uint64_t a = align - 1, i0 = (uint64_t)threadIdx.x * kScanPer;
    uint64_t v[kScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
        v[k] = i0 + k < n ? (((uint64_t)sizes[i0 + k] + a) & ~a) : 0;
        sum += v[k];
    }
    // inclusive scan of the 1 024 partial sums: inside a wavefront with shuffles, over the 16 wavefronts through LDS (round 5: ten
    // Hillis-Steele rounds of two barriers each were most of this one-workgroup kernel's 9 - 12 us)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, off, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), off, 64);
        if ((int)lane >= off) incl += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint64_t wbase = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanBlock / 64; k++) { wbase += k < wave ? sh[k] : 0ull; total += sh[k]; }
    uint64_t run = wbase + incl - sum;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
        if (i0 + k < n) offsets[i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == kScanBlock - 1) offsets[n] = total;
}

#ifndef SPRINTZ_COPY_SMALL_LOG2
#define SPRINTZ_COPY_SMALL_LOG2 5
#endif
// one wavefront per chunk: slot -> dense (LOG2L = 5: half a wavefront per chunk -- slots of at most 2 KB, where a chunk's stream is a few
// hundred bytes and 64 lanes x 16 bytes leave most of the wavefront idle: BASELINE config 1's 440-byte streams, compress 0.434 -> 0.402 ms; a quarter: 0.403)
template <int LOG2L>
__global__ void __launch_bounds__(kThreads) compact_copy_kernel(const uint8_t* slots, uint64_t slot_stride, const uint32_t* sizes,
                                                                const uint64_t* offsets, uint64_t nchunks, uint32_t align,
                                                                uint8_t* dense)
{
    const uint64_t c = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> LOG2L;
    const uint32_t lane = threadIdx.x & ((1u << LOG2L) - 1u);
    if (c >= nchunks) return;
    const uint8_t* s = slots + c * slot_stride;
    uint8_t* d = dense + offsets[c];
    const uint32_t sz = sizes[c];
    if (align == 16) {
        const uint32_t nunits = (sz + 15u) >> 4;     // slots are zero padded to 16
        sprintz::copy_verbatim<false>(s, d, nunits << 4, lane, 1u << LOG2L);      // (four 16-byte loads a lane in flight before its first store)
    } else {
        for (uint32_t j = lane; j < sz; j += 1u << LOG2L) d[j] = s[j];
    }
}

// Chunks too short for one stream group (n < 128 or n < 16 * ndims in the general layout: BASELINE config 3 at 1 KB chunks) are
// their 8-byte header + the samples themselves (sprintz_xff_rle.cpp:116-124, :158-160; encode_kernel.h writes the same bytes
// into a slot).  Every size is known before the launch, so the 16-byte aligned container needs no scan and no slot: one
// wavefront per chunk copies the samples to where they end up -- one pass over the data instead of two.
__global__ void __launch_bounds__(kThreads) verbatim_dense_kernel(const uint8_t* src, uint64_t total_len, uint32_t chunk_len, uint32_t esz, uint32_t D,
                                                                  uint64_t nchunks, uint8_t* dense, uint64_t* offsets, uint32_t* sizes, int64_t* rets)
{
    const uint64_t c = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= nchunks) return;
    const uint64_t first = c * (uint64_t)chunk_len;
    const uint32_t n = (uint32_t)(total_len - first < chunk_len ? total_len - first : chunk_len);
    const uint64_t stride = ((uint64_t)8 + (uint64_t)chunk_len * esz + 15u) & ~(uint64_t)15;     // every chunk but the last is chunk_len long
    const uint32_t size = 8u + n * esz, asize = (size + 15u) & ~15u;
    uint8_t* d = dense + c * stride;
    sprintz::copy_verbatim<true>(src + first * esz, d + 8, n * esz, lane, 64u);
    for (uint32_t j = size + lane; j < asize; j += 64u) d[j] = 0;                                 // the container's alignment padding is zeros
    if (lane == 0) {
        ((uint32_t*)d)[0] = 0;                                                                    // no groups (format.h:36-45)
        ((uint32_t*)d)[1] = (n & 0xffffu) | (D << 16);
        sizes[c] = size;
        if (rets) rets[c] = (int64_t)(size / esz);
        offsets[c] = c * stride;
        if (c == nchunks - 1) offsets[nchunks] = c * stride + asize;
    }
}

// The way back for such batches (chunk_len < 128 or < 16 * ndims: no stream of a valid batch holds a group): one wavefront per
// chunk checks the 8-byte header (no groups, ndims, the tail inside the stream and inside the chunk) and copies the samples --
// instead of decode_kernel.h's whole state machine around the same copy.  A stream that does announce groups cannot be valid
// at this chunk length (one group is 16 * ndims samples) and is SPRINTZ_E_CORRUPT.
__global__ void __launch_bounds__(kThreads) verbatim_decode_kernel(const uint8_t* comp, const uint64_t* offsets, uint64_t nchunks, uint32_t chunk_len,
                                                                   uint32_t esz, uint32_t D, uint8_t* out, int64_t* rets)
{
    const uint64_t c = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= nchunks) return;
    const uint64_t off = offsets[c], slen = offsets[c + 1] - off;
    const uint8_t* s = comp + off;
    bool bad = slen < 8;
    uint32_t remaining = 0;
    if (!bad) {
        const uint32_t w0 = sprintz::load_u32_any(s), w1 = sprintz::load_u32_any(s + 4);
        remaining = w1 & 0xffffu;
        bad = w0 != 0 || (w1 >> 16) != D || remaining > chunk_len || (uint64_t)remaining * esz > slen - 8;
    }
    if (!bad) sprintz::copy_verbatim<true>(s + 8, out + c * (uint64_t)chunk_len * esz, remaining * esz, lane, 64u);
    if (lane == 0 && rets) rets[c] = bad ? sprintz::kErrCorrupt : (int64_t)remaining;
}

}  // namespace

namespace sprintz {
std::atomic<uint64_t> g_dispatch_counts[SPRINTZ_KF_COUNT];      // dispatch.h: which kernel family served a call
int fail(int code, const char* what, hipError_t e)
{
    g_last_error = what;
    if (e != hipSuccess) {
        g_last_error += ": ";
        g_last_error += hipGetErrorString(e);
    }
    return code;
}
int fail_op(int code, const char* op, const char* what)
{
    if (!op) return fail(code, what);
    const std::string named = std::string(op) + ": " + what;
    return fail(code, named.c_str());
}
bool have_device() { return process().have_device; }
int ensure_device()
{
    if (!have_device()) return fail(SPRINTZ_E_NO_DEVICE, "no usable HIP device (libsprintz_mi355x has no CPU fallback)");
    return 0;
}
hipError_t launch_size_scan(const uint32_t* d_sizes, uint64_t n, uint32_t align, uint64_t* d_offsets, void* d_tmp, hipStream_t st)
{
    if (n == 0) return hipMemsetAsync(d_offsets, 0, 8, st);
    if (n <= (uint64_t)kScanOne) {
        hipLaunchKernelGGL(scan_one_kernel, dim3(1), dim3(kScanBlock), 0, st, d_sizes, n, align, d_offsets);
        return hipGetLastError();
    }
    const uint64_t nblocks = (n + kScanBlock - 1) / kScanBlock;
    uint64_t* tmp = (uint64_t*)d_tmp;
    hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)nblocks), dim3(kScanBlock), 0, st, d_sizes, n, align, d_offsets, tmp);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanBlock), 0, st, tmp, nblocks, d_offsets + n);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nblocks), dim3(kScanBlock), 0, st, d_offsets, n, tmp);
    return hipGetLastError();
}

// The lane-per-column decoders' launchers (launch.h): each forwards to the translation unit that holds the instantiation -- the row
// operation's own unit, else the width's.  kDecodeUnits[q][w == 16]
struct DecodeUnit {
    decltype(&decode_generic_w8) generic;
    decltype(&decode_fast_w8) fast;
};
#define SPRINTZ_WIDTH_UNITS {{decode_generic_w8, decode_fast_w8}, {decode_generic_w16, decode_fast_w16}}
#define SPRINTZ_ROW_OP_UNIT_ROW(NAME) {{decode_generic_##NAME, decode_fast_##NAME}, {decode_generic_##NAME, decode_fast_##NAME}},
const DecodeUnit kDecodeUnits[][2] = {SPRINTZ_WIDTH_UNITS, SPRINTZ_WIDTH_UNITS, SPRINTZ_WIDTH_UNITS, SPRINTZ_WIDTH_UNITS,   // kQueryOff .. kQueryWindow
                                      SPRINTZ_ROW_OP_UNITS(SPRINTZ_ROW_OP_UNIT_ROW)};
#undef SPRINTZ_ROW_OP_UNIT_ROW
#undef SPRINTZ_WIDTH_UNITS
static_assert(sizeof(kDecodeUnits) / sizeof(kDecodeUnits[0]) == kQueryFir + 1 && kQueryGather == 4, "a row of units per kQuery* mode");
hipError_t launch_decode_generic(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q < 0 || q > kQueryFir) return hipErrorInvalidValue;
    return kDecodeUnits[q][w == 16].generic(w, fire, lowdim, cpl, q, grid, shmem, st, a);
}
hipError_t launch_decode_fast(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q < 0 || q > kQueryFir) return hipErrorInvalidValue;
    return kDecodeUnits[q][w == 16].fast(w, fire, dp, cpl, exact, q, ds, grid, shmem, st, a);
}
hipError_t launch_decode_uni(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a)
{
    const auto unit = q == kQueryFilter ? decode_uni_filter : w == 8 ? decode_uni_w8 : decode_uni_w16;
    return unit(w, fire, nd, q, grid, st, a);
}

// ---------------------------------------------------------------- launch helpers

int check_common(int codec, int esz, uint16_t ndims)
{
    if (codec < SPRINTZ_CODEC_DELTA || codec > SPRINTZ_CODEC_XFF_NORLE)
        return fail(SPRINTZ_E_INVALID, "codec must be 0 (delta), 1 (xff), 2 (delta, no RLE), 3 (bit-packing only) or 4 (xff, no RLE)");
    if (codec == SPRINTZ_CODEC_XFF_NORLE && esz != 1) return fail(SPRINTZ_E_UNSUPPORTED, "the non-RLE xff codec exists for 8-bit elements only");
    if (esz != 1 && esz != 2) return fail(SPRINTZ_E_INVALID, "elem_bytes must be 1 or 2");
    if (ndims == 0) return fail(SPRINTZ_E_INVALID, "ndims == 0 (reference: sprintz.cpp:36 returns -1)");
    if (ndims > SPRINTZ_MI355X_MAX_NDIMS) return fail(SPRINTZ_E_UNSUPPORTED, "ndims above SPRINTZ_MI355X_MAX_NDIMS");
    return 0;
}

// The stream header's remaining_len is a uint16 (format.h:40): from 4 096 columns on a chunk's verbatim tail -- the whole chunk when
// it is shorter than one group, otherwise at most two blocks (the "<" codecs: sprintz_delta_rle.cpp:226) or one block and the
// ragged rest -- can exceed 65 535 elements.  The reference's single call then writes a header that decodes to a prefix, and the
// drop-in symbols reproduce that; a BATCH that silently loses samples is not acceptable, so the batched entry points refuse it.
int check_batch_tail(uint64_t total_len, uint32_t chunk_len, uint16_t ndims)
{
    if (ndims < 4096 || chunk_len == 0) return 0;
    auto tail_max = [&](uint64_t n) -> uint64_t {
        const uint64_t blk = 8ull * ndims;
        if (n < 128 || n < 2 * blk) return n;
        return n % blk == 0 ? 2 * blk : blk + n % blk;
    };
    const uint64_t last = total_len % chunk_len;
    const bool full = total_len >= chunk_len;
    if ((full && tail_max(chunk_len) > 0xffffu) || (last && tail_max(last) > 0xffffu))
        return fail(SPRINTZ_E_UNSUPPORTED, "a chunk's verbatim tail can exceed the stream header's 16-bit remaining_len at this ndims x chunk_len: the batch would decode to a prefix");
    return 0;
}

// more than 2 047 columns: the column-tiled kernels build the stream with device-scope atomics on the slot and read their own output back
// (any_ndims.hip, "big"): that needs ordinary device memory -- a mapped host or managed buffer is refused instead of producing a damaged stream
static bool is_plain_device_memory(const void* p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

// The dispatch options as ONE exported call sees them: every atomic is loaded once, here, and everything the call decides --
// the host paths' choice between the ticket and the staged form, the planner, the launcher -- uses this copy (plan.h)
Knobs snapshot()
{
    const Process& p = process();
    auto ld = [](const std::atomic<int>& a) { return a.load(std::memory_order_relaxed); };
    return Knobs{ld(p.no_fast), ld(p.lat_chunks), ld(p.blk_chunks), ld(p.blk_kernels), ld(p.enc_pair), ld(p.split_lanes), ld(p.chunks_per_group), ld(p.dense_mode), ld(p.ref_quirk)};
}

// more than 2 047 columns, FIRE: the counters of the column-tiled kernels live in stream-ordered scratch around the launch (any_ndims.hip, "big")
static int alloc_counters(const Plan& p, uint64_t nchunks, int D, hipStream_t st, int32_t** counters)
{
    *counters = nullptr;
    if (p.counters && hipMallocAsync((void**)counters, (size_t)nchunks * (size_t)D * 4, st) != hipSuccess)
        return fail(SPRINTZ_E_HIP, "hipMallocAsync of the counters' scratch (not available during stream capture)");
    return 0;
}

Shape decode_shape(const Batch& b, const void* d_out, const QuerySpec& qs)
{
    Shape s;
    s.codec = b.codec; s.esz = b.esz; s.D = b.ndims; s.nchunks = b.nchunks; s.chunk_len = b.chunk_len;
    s.noheader = qs.noheader; s.q = qs.q; s.general = qs.general; s.col_stride = qs.col_stride; s.host_call = qs.hc != nullptr;
    s.comp_lo = low4(b.comp); s.out_lo = low4(d_out);
    s.capacity = qs.select.capacity;
    s.table_entries = qs.table.entries;
    s.table_row_max = qs.table_row_max;
    s.out_esz = qs.q == kQueryFloat ? float_out_bytes(qs.filter.mode) : 0;
    if (qs.q == kQueryRolling) {                            // the window, the widest output element, and the low bits of every selected output
        s.rows = qs.win.rows;
        s.out_esz = (qs.win.ops & kRollSum) ? 4 : b.esz;
        s.out_lo = low4(qs.win.min) | low4(qs.win.max) | low4(qs.win.sum);
    }
    if (qs.q == kQueryCumulative) {                         // the widest output element (win.count carries sum_bytes) and the low bits of every selected output
        s.out_esz = (qs.win.ops & kCumSum) ? (int)qs.win.count : b.esz;
        s.out_lo = low4(qs.win.min) | low4(qs.win.max) | low4(qs.win.sum);
    }
    if (qs.q == kQueryProject) {                            // the columns of the output and the bytes of one of its elements
        s.rows = qs.filter.mask_stride;
        s.out_esz = project_out_bytes(qs.filter.mode, b.esz);
    }
    if (qs.q == kQueryDerive) {                             // the forms of the output and the bytes of one of its elements
        s.rows = qs.filter.mask_stride;
        s.out_esz = derive_out_bytes(qs.filter.mode);
    }
    if (qs.q == kQueryFir) {                                // the taps (win.rows carries the history's rows, for the ring) and the bytes of an output element
        s.rows = qs.win.count;
        s.out_esz = derive_out_bytes(qs.filter.mode);
    }
    return s;
}

int decode_launch(const Plan& p, const Batch& b, void* d_out, int64_t* d_rets, hipStream_t st, const QuerySpec& qs)
{
    // (the host paths hand over the plan they chose the ticket form by: not reached from there)
    if (qs.hc && p.family != SPRINTZ_KF_DEC_LAT) return fail(SPRINTZ_E_HIP, "internal: host call on a kernel that cannot end it");
    // more than 2 047 columns: the column-tiled kernels build the stream with device-scope atomics on the slot and read their own output back
    if (p.plain_memory && !is_plain_device_memory(d_out)) return fail(SPRINTZ_E_INVALID, "more than 2047 columns: the output must be device memory (hipMalloc), not mapped host or managed memory");
    if (p.err) return fail(p.err, p.what);

    DecodeArgs a{};
    a.comp = (const uint8_t*)b.comp;
    a.offsets = b.offsets;
    a.nchunks = b.nchunks;
    a.chunk_len = b.chunk_len;
    a.D = b.ndims;
    a.log2DP = p.log2DP;
    a.out = d_out;
    a.rets = d_rets;
    a.noheader = qs.noheader;
    a.nh_ngroups = qs.nh_ngroups;
    a.nh_remaining = qs.nh_remaining;
    a.chunks_per_group = p.chunks_per_group;
    a.qop = qs.qop;
    a.qres = qs.qres;
    a.win = qs.win;
    a.gather = qs.gather;
    a.filter = qs.filter;
    a.select = qs.select;
    a.rows = qs.rows;
    a.table = qs.table;
    a.table.table_off = p.table_off;
    a.table.wg_chunks = p.wg_chunks;
    a.hist = qs.hist;
    a.mom = qs.mom;
    a.gby = qs.gby;
    a.ext = qs.ext;
    a.lin = qs.lin;
    a.norle = p.norle;
    a.raw = p.raw;
    a.col_stride = qs.col_stride;
    a.quirk = p.quirk;
    a.vec_store = p.vec_store;
    a.lds_group_stride = p.lds_group_stride;

    const int w = 8 * b.esz;
    const unsigned grid = (unsigned)p.grid;
    hipError_t e = hipSuccess;
    const char* what = "";
    switch (p.family) {
    case SPRINTZ_KF_DEC_BIG: {
        int32_t* counters;
        if (int rc = alloc_counters(p, b.nchunks, b.ndims, st, &counters)) return rc;
        e = launch_decode_big(w, p.counters, grid, st, a, counters);
        if (counters) (void)hipFreeAsync(counters, st);
        what = "decode_big kernel launch";
        break;
    }
    case SPRINTZ_KF_DEC_ANY: what = "decode_any kernel launch"; e = launch_decode_any(w, p.fire, grid, st, a); break;
    case SPRINTZ_KF_DEC_VERBATIM:
        what = "hipGetLastError()";
        hipLaunchKernelGGL(verbatim_decode_kernel, dim3(grid), dim3(kThreads), 0, st, a.comp, a.offsets, a.nchunks, a.chunk_len,
                           (uint32_t)b.esz, (uint32_t)b.ndims, (uint8_t*)d_out, d_rets);
        e = hipGetLastError();
        break;
    case SPRINTZ_KF_DEC_LAT:
        what = "decode_lat kernel launch";
        if (qs.hc) { a.offsets = nullptr; a.one_off0 = qs.hc->off0; a.one_off1 = qs.hc->off1; a.host_flag = qs.hc->flag; a.host_ticket = qs.hc->ticket; }
        e = launch_decode_lat(w, p.fire, p.dp, p.lowdim, grid, p.lat_bound, st, a);
        break;
    case SPRINTZ_KF_DEC_ROW: what = "decode_row kernel launch"; e = launch_decode_row(w, grid, st, a, p.row); break;
    case SPRINTZ_KF_DEC_BLK: what = "decode_blk kernel launch"; e = launch_decode_blk(w, grid, st, a, p.blkd); break;
    case SPRINTZ_KF_DEC_FAST:
    case SPRINTZ_KF_GATHER_FAST:
        what = p.family == SPRINTZ_KF_GATHER_FAST ? "decode_fast gather kernel launch" : "decode_fast kernel launch";
        e = launch_decode_fast(w, p.fire, p.dp, p.cpl, p.exact, qs.q, p.ds, grid, (size_t)p.lds, st, a);
        break;
    case SPRINTZ_KF_DEC_UNI: what = "decode_uni kernel launch"; e = launch_decode_uni(w, p.fire, b.ndims, qs.q, grid, st, a); break;
    default:
        what = p.family == SPRINTZ_KF_GATHER_GENERIC ? "decode gather kernel launch" : "decode kernel launch";
        e = launch_decode_generic(w, p.fire, p.lowdim, p.cpl, qs.q, grid, (size_t)p.lds, st, a);
        break;
    }
    if (e != hipSuccess) return fail(SPRINTZ_E_HIP, what, e);
    dispatched(p.family);
    return 0;
}

int decode_batch(const Knobs& k, const Batch& b, void* d_out, int64_t* d_rets, hipStream_t st, const QuerySpec& qs)
{
    if (b.nchunks == 0) return 0;
    return decode_launch(plan_decode(decode_shape(b, d_out, qs), k), b, d_out, d_rets, st, qs);
}

Shape encode_shape(const EncodeBatch& j, bool dense, bool host_call)
{
    Shape s;
    s.codec = j.codec; s.esz = j.esz; s.D = j.ndims; s.total_len = j.total_len; s.nchunks = sprintz_mi355x_num_chunks(j.total_len, j.chunk_len); s.chunk_len = j.chunk_len;
    s.general = j.general; s.col_stride = j.col_stride; s.write_size = j.write_size; s.dense = dense; s.host_call = host_call;
    s.src_lo = low4(j.src); s.slots_lo = low4(j.slots); s.slot_stride = j.slot_stride;
    if (j.fsrc) { s.q = kQueryFloat; s.out_esz = float_out_bytes(j.q_mode); }
    return s;
}

int encode_launch(const Plan& p, const EncodeBatch& j, hipStream_t st, const DenseRequest* dense, const HostCall* hc)
{
    // (the host paths hand over the plan they chose the ticket form by: not reached from there)
    if (hc && p.family != SPRINTZ_KF_ENC_LAT) return fail(SPRINTZ_E_HIP, "internal: host call on a kernel that cannot end it");
    if (p.plain_memory && !is_plain_device_memory(j.slots)) return fail(SPRINTZ_E_INVALID, "more than 2047 columns: the slots must be device memory (hipMalloc), not mapped host or managed memory");
    if (p.err) return fail(p.err, p.what);
    const int esz = j.esz, ndims = j.ndims;

    EncodeArgs a{};
    a.src = j.src;
    a.total_len = j.total_len;
    a.chunk_len = j.chunk_len;
    a.nchunks = sprintz_mi355x_num_chunks(j.total_len, j.chunk_len);
    a.D = j.ndims;
    a.log2DP = p.log2DP;
    a.slots = (uint8_t*)j.slots;
    a.slot_stride = j.slot_stride;
    a.sizes = j.sizes;
    a.rets = j.rets;
    a.write_size = j.write_size;
    a.col_stride = j.col_stride;
    a.norle = p.norle;
    a.raw = p.raw;
    a.cap = p.cap;
    a.lds_group_stride = p.lds_group_stride;
    a.q_inv = j.q_inv;
    a.q_off = j.q_off;
    a.q_mode = j.q_mode;
    if (p.fused) {
        a.dn.dense = (uint8_t*)dense->d_dense;
        a.dn.offsets = dense->d_offsets;
        a.dn.wg_state = (uint64_t*)dense->d_tmp;
        a.dn.grid = (uint32_t)p.grid;
        HIP_TRY(hipMemsetAsync(dense->d_tmp, 0, ((size_t)p.grid + 1) * sizeof(uint64_t), st));   // look-back words + the ticket counter
    }

    const int w = 8 * esz;
    const unsigned grid = (unsigned)p.grid;
    hipError_t e = hipSuccess;
    const char* what = "";
    if (j.fsrc) {                                           // a float source: the planner names no other family for one
        if (p.family != SPRINTZ_KF_ENC_PAIR && p.family != SPRINTZ_KF_ENC_WIDE && p.family != SPRINTZ_KF_ENC_SPLIT && p.family != SPRINTZ_KF_ENC_GENERIC)
            return fail(SPRINTZ_E_HIP, "internal: a float source on a kernel that cannot quantise");
        e = esz == 1 ? launch_encode_float_w8(p.family, p.fire, p.lowdim, p.cpl, p.dp, p.exact, grid, (size_t)p.lds, st, a)
                     : launch_encode_float_w16(p.family, p.fire, p.lowdim, p.cpl, p.dp, p.exact, grid, (size_t)p.lds, st, a);
        if (e != hipSuccess) return fail(SPRINTZ_E_HIP, "encode kernel launch (float source)", e);
        dispatched(p.family);
        return 0;
    }
    switch (p.family) {
    case SPRINTZ_KF_ENC_BIG: {
        int32_t* counters;
        if (int rc = alloc_counters(p, a.nchunks, ndims, st, &counters)) return rc;
        e = launch_encode_big(w, p.counters, grid, st, a, counters);
        if (counters) (void)hipFreeAsync(counters, st);
        what = "encode_big kernel launch";
        break;
    }
    case SPRINTZ_KF_ENC_ANY: what = "encode_any kernel launch"; e = launch_encode_any(w, p.fire, grid, (size_t)p.lds, st, a); break;
    case SPRINTZ_KF_ENC_LAT:
        what = "encode_lat kernel launch";
        if (hc) { a.host_flag = hc->flag; a.host_ticket = hc->ticket; }
        e = launch_encode_lat(w, p.fire, p.dp, p.lowdim, grid, p.lat_bound, st, a);
        break;
    case SPRINTZ_KF_ENC_BLK: what = "encode_blk kernel launch"; e = launch_encode_blk(w, grid, st, a, p.blke); break;
    case SPRINTZ_KF_ENC_BLK_UNI: what = "encode_blk_uni kernel launch"; e = launch_encode_blk_uni(w, grid, st, a, p.blke); break;
    case SPRINTZ_KF_ENC_PAIR: {
        // (experiment knob: extra, unused LDS a workgroup claims -- fewer resident waves; what occupancy is worth to this loop: DESIGN 4.4)
        static const size_t lds_pad = getenv("SPRINTZ_MI355X_ENC_LDS_PAD") ? (size_t)atol(getenv("SPRINTZ_MI355X_ENC_LDS_PAD")) : 0;
        e = esz == 1 ? launch_encode_pair_w8(p.fire, p.dp, p.exact, grid, (size_t)p.lds + lds_pad, st, a)
                     : launch_encode_pair_w16(p.fire, p.dp, p.exact, grid, (size_t)p.lds + lds_pad, st, a);
        what = "encode_wide (pair) kernel launch";
        break;
    }
    case SPRINTZ_KF_ENC_FAST:
        what = "encode_fast kernel launch";
        e = esz == 1 ? launch_encode_fast_w8(p.fire, p.dp, p.exact, grid, (size_t)p.lds, st, a) : launch_encode_fast_w16(p.fire, p.dp, p.exact, grid, (size_t)p.lds, st, a);
        break;
    case SPRINTZ_KF_ENC_SPLIT: what = "encode_wide kernel launch"; e = launch_encode_split_w8(p.fire, grid, (size_t)p.lds, st, a); break;
    case SPRINTZ_KF_ENC_WIDE:
        what = "encode_wide kernel launch";
        e = esz == 1 ? launch_encode_wide_w8(p.fire, p.exact, grid, (size_t)p.lds, st, a) : launch_encode_wide_w16(p.fire, p.exact, grid, (size_t)p.lds, st, a);
        break;
    case SPRINTZ_KF_ENC_UNI: what = "encode_uni kernel launch"; e = esz == 1 ? launch_encode_uni_w8(p.fire, ndims, grid, st, a) : launch_encode_uni_w16(p.fire, ndims, grid, st, a); break;
    default: what = "encode kernel launch"; e = esz == 1 ? launch_encode_w8(p.fire, p.lowdim, p.cpl, grid, (size_t)p.lds, st, a) : launch_encode_w16(p.fire, p.lowdim, p.cpl, grid, (size_t)p.lds, st, a); break;
    }
    if (e != hipSuccess) return fail(SPRINTZ_E_HIP, what, e);
    dispatched(p.family);
    return 0;
}

int encode_batch(const Knobs& k, const EncodeBatch& j, hipStream_t st)
{
    if (sprintz_mi355x_num_chunks(j.total_len, j.chunk_len) == 0) return 0;
    return encode_launch(plan_encode(encode_shape(j, false, false), k), j, st);
}

}  // namespace sprintz

namespace {

// ---- what the batched encoding calls check and end alike
// the source, the slots and -- dense != null -- the container the call builds; `misaligned`: the call's own words
int check_slots(const EncodeBatch& j, const DenseRequest* dense, const char* misaligned)
{
    if (!j.src || !j.slots || !j.sizes || (dense && (!dense->d_dense || !dense->d_offsets || !dense->d_tmp))) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if (j.slot_stride % 16 || (uintptr_t)j.slots % 16 || (dense && ((uintptr_t)dense->d_dense % 16 || (uintptr_t)dense->d_tmp % 8)))
        return fail(SPRINTZ_E_INVALID, misaligned);
    if (j.slot_stride < sprintz_mi355x_compress_bound(j.esz, j.chunk_len, j.ndims)) return fail(SPRINTZ_E_INVALID, "slot_stride below sprintz_mi355x_compress_bound");
    return 0;
}

// the column-major calls, in front of their own checks: `rows` is what col_stride must hold, `short_stride` the refusal
int check_colmajor(int codec, int esz, uint16_t ndims, uint32_t rows_per_chunk, uint64_t col_stride, uint64_t rows, const char* short_stride)
{
    if (int rc = check_common(codec, esz, ndims)) return rc;
    if (rows_per_chunk == 0 || (uint64_t)rows_per_chunk * ndims > (1u << 30)) return fail(SPRINTZ_E_INVALID, "rows_per_chunk * ndims must be in 1..2^30");
    if (col_stride < rows) return fail(SPRINTZ_E_INVALID, short_stride);
    return 0;
}

// the tail of the *_dense calls: the encoder `enc` planned; where it has no dense tail (low-dim, more than 64 columns,
// misaligned blocks, a column-major source) the two-launch path behind it
int encode_dense(const Plan& enc, const EncodeBatch& j, const DenseRequest& dr, uint64_t nchunks, void* hip_stream)
{
    const int rc = encode_launch(enc, j, (hipStream_t)hip_stream, &dr);
    if (!rc && enc.fused) dispatched(SPRINTZ_KF_DENSE_FUSED);
    if (rc || enc.fused) return rc;
    return sprintz_mi355x_compact(j.slots, j.slot_stride, j.sizes, nchunks, 16, dr.d_dense, dr.d_offsets, dr.d_tmp, hip_stream);
}

}  // namespace

// =============================================================== exported C-ABI
extern "C" {

int sprintz_mi355x_abi_version(void) { return SPRINTZ_MI355X_ABI_VERSION; }

int sprintz_mi355x_set_option(int option, int value)
{
    if (std::atomic<long long>* huf0 = huf0_option(option)) {
        if (value < 0) return fail(SPRINTZ_E_INVALID, kNotNegative);
        *huf0 = value;
        return 0;
    }
    for (const Option& o : kOptions) {
        if (o.id != option) continue;
        if (o.outside && (value < o.lo || value > o.hi)) return fail(SPRINTZ_E_INVALID, o.outside);
        process().*o.knob = o.outside ? value : value != 0;
        return 0;
    }
    return fail(SPRINTZ_E_INVALID, "unknown option");
}
int sprintz_mi355x_get_option(int option)
{
    if (std::atomic<long long>* huf0 = huf0_option(option)) return (int)huf0->load(std::memory_order_relaxed);
    for (const Option& o : kOptions)
        if (o.id == option) return (process().*o.knob).load(std::memory_order_relaxed);
    return fail(SPRINTZ_E_INVALID, "unknown option");
}
const char* sprintz_mi355x_last_error(void) { return g_last_error.c_str(); }

int sprintz_mi355x_dispatch_counts(uint64_t* counts, int capacity)
{
    for (int k = 0; counts && k < capacity && k < SPRINTZ_KF_COUNT; k++) counts[k] = sprintz::g_dispatch_counts[k].load(std::memory_order_relaxed);
    return SPRINTZ_KF_COUNT;
}
const char* sprintz_mi355x_dispatch_name(int family)
{
    return family >= 0 && family < SPRINTZ_KF_COUNT ? kFamilyNames[family] : nullptr;
}

size_t sprintz_mi355x_compress_bound(int elem_bytes, uint32_t chunk_len, uint16_t ndims) { return compress_bound(elem_bytes, chunk_len, ndims); }

uint64_t sprintz_mi355x_num_chunks(uint64_t total_len, uint32_t chunk_len)
{
    if (chunk_len == 0) return 0;
    return (total_len + chunk_len - 1) / chunk_len;
}

int sprintz_mi355x_compress_batch(int codec, int elem_bytes, const void* d_src, uint64_t total_len, uint32_t chunk_len,
                                  uint16_t ndims, void* d_slots, size_t slot_stride, uint32_t* d_sizes, int64_t* d_rets,
                                  void* hip_stream)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (chunk_len == 0 || chunk_len > (1u << 30)) return fail(SPRINTZ_E_INVALID, "chunk_len must be in 1..2^30");
    const EncodeBatch j{codec, elem_bytes, d_src, total_len, chunk_len, ndims, d_slots, slot_stride, d_sizes, d_rets};
    if ((rc = check_slots(j, nullptr, "slots must be 16-byte aligned/strided"))) return rc;
    if ((rc = check_batch_tail(total_len, chunk_len, ndims))) return rc;
    if ((rc = ensure_device())) return rc;
    return encode_batch(snapshot(), j, (hipStream_t)hip_stream);
}

size_t sprintz_mi355x_compress_dense_tmp_bytes(uint64_t nchunks)
{
    // the chained scan's word per workgroup (at most nchunks / 4 workgroups: a chunk takes at most 64 of a workgroup's 256
    // lanes) + the ticket counter -- or the two-launch path's scan scratch, whichever is larger
    const size_t a = (size_t)(nchunks / 4 + 2) * sizeof(uint64_t), b = sprintz_mi355x_compact_tmp_bytes(nchunks);
    return a > b ? a : b;
}

int sprintz_mi355x_compress_batch_dense(int codec, int elem_bytes, const void* d_src, uint64_t total_len, uint32_t chunk_len,
                                        uint16_t ndims, void* d_slots, size_t slot_stride, uint32_t* d_sizes, int64_t* d_rets,
                                        void* d_dense, uint64_t* d_offsets, void* d_tmp, void* hip_stream)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (chunk_len == 0 || chunk_len > (1u << 30)) return fail(SPRINTZ_E_INVALID, "chunk_len must be in 1..2^30");
    const EncodeBatch j{codec, elem_bytes, d_src, total_len, chunk_len, ndims, d_slots, slot_stride, d_sizes, d_rets};
    const DenseRequest dr{d_dense, d_offsets, d_tmp};
    if ((rc = check_slots(j, &dr, "slots and the container must be 16-byte aligned/strided"))) return rc;
    if ((rc = check_batch_tail(total_len, chunk_len, ndims))) return rc;
    if ((rc = ensure_device())) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t nchunks = sprintz_mi355x_num_chunks(total_len, chunk_len);
    if (nchunks == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, st));
        return 0;
    }
    Plan enc;                                               // (stays empty where the verbatim kernel takes the batch)
    const Plan dp = plan_dense(encode_shape(j, false, false), snapshot(), &enc);
    if (dp.err && !enc.err) return fail(dp.err, dp.what);   // (the encoder's own refusal is encode_launch's to report, behind the checks it makes first)
    if (dp.family == SPRINTZ_KF_DENSE_VERBATIM) {
        hipLaunchKernelGGL(verbatim_dense_kernel, dim3((unsigned)dp.grid), dim3(kThreads), 0, st, (const uint8_t*)d_src, total_len, chunk_len,
                           (uint32_t)elem_bytes, (uint32_t)ndims, nchunks, (uint8_t*)d_dense, d_offsets, d_sizes, d_rets);
        HIP_TRY(hipGetLastError());
        dispatched(SPRINTZ_KF_DENSE_VERBATIM);
        return 0;
    }
    return encode_dense(enc, j, dr, nchunks, hip_stream);
}

// ---- a float source, quantised inside the encoder (quant.h)
namespace {
// every refusal of the two calls below carries the call's name
int named(const char* op, int rc)
{
    if (rc && g_last_error.rfind(op, 0) != 0) g_last_error = std::string(op) + ": " + g_last_error;
    return rc;
}
// the checks the two calls share, before the device is touched; fills the float side of j
int check_float_source(const char* op, EncodeBatch& j, int src_format, const float* d_inv_scale, const float* d_offset, uint32_t flags, const DenseRequest* dense)
{
    int rc = check_common(j.codec, j.esz, j.ndims);
    if (rc) return named(op, rc);
    if (j.chunk_len == 0 || j.chunk_len > (1u << 30)) return fail_op(SPRINTZ_E_INVALID, op, "chunk_len must be in 1..2^30");
    if (j.chunk_len % j.ndims) return fail_op(SPRINTZ_E_INVALID, op, "chunk_len must be a multiple of ndims (element e of a chunk is in column e % ndims)");
    static_assert(SPRINTZ_FLOAT_F32 == (int)kFloatF32 && SPRINTZ_FLOAT_F16 == (int)kFloatF16 && SPRINTZ_FLOAT_BF16 == (int)kFloatBF16, "the format travels as it is given");
    if (src_format != SPRINTZ_FLOAT_F32 && src_format != SPRINTZ_FLOAT_F16 && src_format != SPRINTZ_FLOAT_BF16)
        return fail_op(SPRINTZ_E_INVALID, op, "src_format must be SPRINTZ_FLOAT_F32, SPRINTZ_FLOAT_F16 or SPRINTZ_FLOAT_BF16");
    if (flags & ~(uint32_t)(SPRINTZ_FLOAT_SIGNED | SPRINTZ_QUANT_FLOOR)) return fail_op(SPRINTZ_E_INVALID, op, "unknown flag");
    j.fsrc = true;
    j.q_inv = d_inv_scale;
    j.q_off = d_offset;
    j.q_mode = (uint32_t)src_format | ((flags & SPRINTZ_FLOAT_SIGNED) ? kFloatSignedBit : 0u) | ((flags & SPRINTZ_QUANT_FLOOR) ? kQuantFloorBit : 0u);
    if (j.ndims > 512) return fail_op(SPRINTZ_E_UNSUPPORTED, op, "more than 512 columns");
    if (j.codec != SPRINTZ_CODEC_DELTA && j.codec != SPRINTZ_CODEC_XFF) return fail_op(SPRINTZ_E_UNSUPPORTED, op, "the RLE codecs (delta, xff) only");
    if ((rc = check_slots(j, dense, dense ? "slots and the container must be 16-byte aligned/strided" : "slots must be 16-byte aligned/strided"))) return named(op, rc);
    if ((uintptr_t)j.src % (uintptr_t)float_out_bytes(j.q_mode)) return fail_op(SPRINTZ_E_INVALID, op, "d_src must be aligned to the source element size");
    if ((uintptr_t)d_inv_scale % 4 || (uintptr_t)d_offset % 4) return fail_op(SPRINTZ_E_INVALID, op, "d_inv_scale and d_offset must be 4-byte aligned");
    if ((rc = check_batch_tail(j.total_len, j.chunk_len, j.ndims))) return named(op, rc);
    return 0;
}
}  // namespace

int sprintz_mi355x_compress_batch_float(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale, const float* d_offset,
                                        uint32_t flags, uint64_t total_len, uint32_t chunk_len, uint16_t ndims, void* d_slots, size_t slot_stride,
                                        uint32_t* d_sizes, int64_t* d_rets, void* hip_stream)
{
    static const char* const op = "compress_batch_float";
    EncodeBatch j{codec, elem_bytes, d_src, total_len, chunk_len, ndims, d_slots, slot_stride, d_sizes, d_rets};
    int rc = check_float_source(op, j, src_format, d_inv_scale, d_offset, flags, nullptr);
    if (rc) return rc;
    if (total_len == 0) return 0;
    if ((rc = ensure_device())) return named(op, rc);
    return named(op, encode_batch(snapshot(), j, (hipStream_t)hip_stream));
}

int sprintz_mi355x_compress_batch_float_dense(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale, const float* d_offset,
                                              uint32_t flags, uint64_t total_len, uint32_t chunk_len, uint16_t ndims, void* d_slots, size_t slot_stride,
                                              uint32_t* d_sizes, int64_t* d_rets, void* d_dense, uint64_t* d_offsets, void* d_tmp, void* hip_stream)
{
    static const char* const op = "compress_batch_float_dense";
    EncodeBatch j{codec, elem_bytes, d_src, total_len, chunk_len, ndims, d_slots, slot_stride, d_sizes, d_rets};
    const DenseRequest dr{d_dense, d_offsets, d_tmp};
    int rc = check_float_source(op, j, src_format, d_inv_scale, d_offset, flags, &dr);
    if (rc) return rc;
    if (total_len == 0) return 0;
    if ((rc = ensure_device())) return named(op, rc);
    Plan enc;
    const Plan dp = plan_dense(encode_shape(j, false, false), snapshot(), &enc);       // (never the verbatim kernel: it copies raw source bytes)
    if (dp.err && !enc.err) return fail_op(dp.err, op, dp.what);
    return named(op, encode_dense(enc, j, dr, sprintz_mi355x_num_chunks(total_len, chunk_len), hip_stream));
}

size_t sprintz_mi355x_compact_tmp_bytes(uint64_t nchunks)
{
    return (size_t)((nchunks + kScanBlock - 1) / kScanBlock + 1) * sizeof(uint64_t);
}

int sprintz_mi355x_compact(const void* d_slots, size_t slot_stride, const uint32_t* d_sizes, uint64_t nchunks, uint32_t align,
                           void* d_dense, uint64_t* d_offsets, void* d_scan_tmp, void* hip_stream)
{
    if (align == 0 || align > 16 || (align & (align - 1))) return fail(SPRINTZ_E_INVALID, "align must be a power of two <= 16");
    if (!d_slots || !d_sizes || !d_dense || !d_offsets || !d_scan_tmp) return fail(SPRINTZ_E_INVALID, "null device pointer");
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (nchunks == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, st));
        return 0;
    }
    // (round 6: scan AND copy in one launch -- a workgroup per 64 chunks, wave 0 scanning their sizes and finding its place by compact_tail.h's
    //  chained scan, then the waves copying -- was built and measured: BASELINE config 3 at 10 KB 0.291 against 0.271 ms for the whole compress call,
    //  config 1 0.466 against 0.390: the tickets and the look-back cost more than the three ~5 us scan launches they replace.  Not kept.)
    HIP_TRY(launch_size_scan(d_sizes, nchunks, align, d_offsets, d_scan_tmp, st));
    const int log2l = slot_stride <= 2048 ? SPRINTZ_COPY_SMALL_LOG2 : 6;                           // lanes a chunk (compact_copy_kernel)
    const uint64_t grid = ((nchunks << log2l) + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(log2l == 6 ? compact_copy_kernel<6> : compact_copy_kernel<SPRINTZ_COPY_SMALL_LOG2>, dim3((unsigned)grid), dim3(kThreads), 0, st,
                       (const uint8_t*)d_slots, (uint64_t)slot_stride, d_sizes, d_offsets, nchunks, align, (uint8_t*)d_dense);
    HIP_TRY(hipGetLastError());
    dispatched(SPRINTZ_KF_DENSE_COMPACT);
    return 0;
}

int sprintz_mi355x_decompress_batch(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                    uint32_t chunk_len, uint16_t ndims, void* d_out, int64_t* d_rets, void* hip_stream)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (chunk_len == 0) return fail(SPRINTZ_E_INVALID, "chunk_len == 0");
    if (!d_comp || !d_offsets || !d_out) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if ((rc = ensure_device())) return rc;
    return decode_batch(Batch{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims}, d_out, d_rets, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------- column-major matrices (BASELINE config 5)
int sprintz_mi355x_compress_batch_colmajor(int codec, int elem_bytes, const void* d_src, uint64_t nrows, uint64_t col_stride,
                                           uint32_t rows_per_chunk, uint16_t ndims, void* d_slots, size_t slot_stride,
                                           uint32_t* d_sizes, int64_t* d_rets, void* hip_stream)
{
    int rc = check_colmajor(codec, elem_bytes, ndims, rows_per_chunk, col_stride, nrows, "col_stride < nrows");
    if (rc) return rc;
    const EncodeBatch j{codec, elem_bytes, d_src, nrows * (uint64_t)ndims, rows_per_chunk * (uint32_t)ndims, ndims, d_slots, slot_stride, d_sizes, d_rets, 1, col_stride};
    if ((rc = check_slots(j, nullptr, "slots must be 16-byte aligned/strided"))) return rc;
    if ((rc = ensure_device())) return rc;
    return encode_batch(snapshot(), j, (hipStream_t)hip_stream);
}

int sprintz_mi355x_compress_batch_colmajor_dense(int codec, int elem_bytes, const void* d_src, uint64_t nrows, uint64_t col_stride,
                                                 uint32_t rows_per_chunk, uint16_t ndims, void* d_slots, size_t slot_stride,
                                                 uint32_t* d_sizes, int64_t* d_rets, void* d_dense, uint64_t* d_offsets, void* d_tmp,
                                                 void* hip_stream)
{
    int rc = check_colmajor(codec, elem_bytes, ndims, rows_per_chunk, col_stride, nrows, "col_stride < nrows");
    if (rc) return rc;
    const EncodeBatch j{codec, elem_bytes, d_src, nrows * (uint64_t)ndims, rows_per_chunk * (uint32_t)ndims, ndims, d_slots, slot_stride, d_sizes, d_rets, 1, col_stride};
    const DenseRequest dr{d_dense, d_offsets, d_tmp};
    if ((rc = check_slots(j, &dr, "slots and the container must be 16-byte aligned/strided, d_tmp 8-byte aligned"))) return rc;
    if ((rc = ensure_device())) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t nchunks = sprintz_mi355x_num_chunks(j.total_len, j.chunk_len);
    if (nchunks == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, st));
        return 0;
    }
    // (a column-major source never carries the container's tail -- plan.h, plan_encode -- so this is the two-launch path today)
    const Knobs knobs = snapshot();
    return encode_dense(plan_encode(encode_shape(j, knobs.dense_mode != 0, false), knobs), j, dr, nchunks, hip_stream);
}

int sprintz_mi355x_decompress_batch_colmajor(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets,
                                             uint64_t nchunks, uint32_t rows_per_chunk, uint16_t ndims, uint64_t col_stride,
                                             void* d_out, int64_t* d_rets, void* hip_stream)
{
    int rc = check_colmajor(codec, elem_bytes, ndims, rows_per_chunk, col_stride, nchunks * (uint64_t)rows_per_chunk, "col_stride < nchunks * rows_per_chunk");
    if (rc) return rc;
    if (!d_comp || !d_offsets || !d_out) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if ((rc = ensure_device())) return rc;
    QuerySpec qs;
    qs.col_stride = col_stride;
    return decode_batch(Batch{codec, elem_bytes, d_comp, d_offsets, nchunks, rows_per_chunk * (uint32_t)ndims, ndims}, d_out, d_rets, (hipStream_t)hip_stream, qs);
}

}  // extern "C"
