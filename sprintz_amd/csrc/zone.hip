// zone.hip -- zone-map pruning around the filter launches (zone.h holds the rules): classify every chunk from its per-column minimum
// and maximum, compact the offsets of the chunks that still need the decoder into a container of their own, and expand a filter's
// compact results back into filter_rows' layout.  Three small kernels and the size scan between the first two; none of them reads
// the container, belongs to a decode family or touches an existing kernel.
#include "../../include/sprintz_mi355x.h"

#include <hip/hip_runtime.h>

#include <string>

#include "entry.h"
#include "zone.h"

namespace sprintz {
namespace {

// the predicate of one prune call, as the classify kernel takes it (box: lo / hi arrays of the element type; linear: weights and the interval)
struct ZonePredicate {
    const void* lo;
    const void* hi;
    const int32_t* w;
    uint32_t mode;
    int32_t bias, lin_lo, lin_hi;
};

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int off, int G)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, G), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), off, G);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Classify.  A group of G = 2^log2G lanes a chunk (as many as it has columns, 64 at the most): the lanes take the chunk's columns in turn,
// fold zone.h's per-column verdicts and combine them with butterflies over the group; lane 0 writes the class and the flag the scan
// adds up.  Whole groups leave together.
template <typename T, bool LINEAR>
__global__ void __launch_bounds__(kThreads) zone_classify_kernel(uint64_t nchunks, uint32_t chunk_len, uint32_t D, int log2G, const uint64_t* offsets,
                                                                 const T* zmin, const T* zmax, const int64_t* zlen, ZonePredicate p,
                                                                 uint8_t* cls, uint32_t* flags)
{
    const int G = 1 << log2G;
    const uint64_t gtid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & (uint32_t)(G - 1);
    const uint64_t c = gtid >> log2G;
    if (c >= nchunks) return;
    const bool too_wide = zone_span_too_wide(offsets[0], offsets[nchunks]);
    const int by_len = zone_class_by_len(zlen[c], chunk_len, D, too_wide);
    const T* mn = zmin + c * (uint64_t)D;
    const T* mx = zmax + c * (uint64_t)D;
    uint8_t k;
    if constexpr (LINEAR) {
        int64_t smin = 0, smax = 0;
        for (uint32_t d = lane; d < D; d += (uint32_t)G) {
            const int32_t w = p.w[d];
            smin += zone_linear_min_term(w, mn[d], mx[d]);
            smax += zone_linear_max_term(w, mn[d], mx[d]);
        }
        for (int off = 1; off < G; off <<= 1) {
            smin += shfl_xor_i64(smin, off, G);
            smax += shfl_xor_i64(smax, off, G);
        }
        k = zone_linear_class(smin + p.bias, smax + p.bias, p.lin_lo, p.lin_hi);
    } else {
        const T* lo = (const T*)p.lo;
        const T* hi = (const T*)p.hi;
        uint32_t some = 0, every = kZoneDisjoint | kZoneInside;
        for (uint32_t d = lane; d < D; d += (uint32_t)G) {
            const uint32_t v = zone_box_column(mn[d], mx[d], lo[d], hi[d]);
            some |= v;
            every &= v;
        }
        for (int off = 1; off < G; off <<= 1) {
            some |= (uint32_t)__shfl_xor((int)some, off, G);
            every &= (uint32_t)__shfl_xor((int)every, off, G);
        }
        k = zone_box_class(some, every, p.mode);
    }
    if (by_len >= 0) k = (uint8_t)by_len;
    if (lane == 0) {
        cls[c] = k;
        flags[c] = k == kZoneDecode ? 1u : 0u;
    }
}

// Compact.  pos = the exclusive scan of the flags, pos[nchunks] = n' the survivors.  Thread i <= nchunks: a surviving chunk i puts its offset
// at place pos[i] (< n'), and place i itself, where it lies at or behind n', takes the container's end -- every entry of surv has one
// writer, the order is the batch's, and no atomic decides a place.
__global__ void __launch_bounds__(kThreads) zone_compact_kernel(uint64_t nchunks, const uint64_t* offsets, const uint8_t* cls, const uint64_t* pos, uint64_t* surv)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > nchunks) return;
    if (i < nchunks && cls[i] == kZoneDecode) surv[pos[i]] = offsets[i];
    if (i >= pos[nchunks]) surv[i] = offsets[nchunks];
}

// Expand.  Thread t takes the four mask bytes of one ALIGNED dword of the destination (the mask may start anywhere, and a chunk's row of
// MB bytes has any alignment) and, where t < nchunks, chunk t's count and ret.  A byte of a decoded chunk comes from the chunk's slot in
// the compact mask, a byte of any other chunk from its class and its rows; a dword that lies inside the mask is one store, the two at
// its ends go out bytewise.  Every byte has one writer.
__global__ void __launch_bounds__(kThreads) zone_expand_kernel(uint64_t nchunks, uint32_t chunk_len, uint32_t D, uint32_t MB, const uint8_t* cls,
                                                               const uint64_t* pos, const int64_t* zlen, const uint8_t* cmask, const uint32_t* ccounts,
                                                               const int64_t* crets, uint8_t* mask, uint32_t* counts, int64_t* rets)
{
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < nchunks) {
        const uint8_t k = cls[t];
        const int64_t n = zlen[t];
        if (k == kZoneDecode) {
            const uint64_t s = pos[t];
            if (counts) counts[t] = ccounts[s];
            // a chunk the zone map found damaged keeps the map's code: a truncated stream is told by its length alone (decode_fast.h), and
            // in the survivors' container its length runs on to the next survivor, over the bytes of the chunks skipped between them
            if (rets) rets[t] = n < 0 ? n : crets[s];
        } else {
            if (counts) counts[t] = k == kZoneAll ? zone_rows(n, chunk_len, D) : 0u;
            if (rets) rets[t] = n;
        }
    }
    if (!mask) return;
    const uint64_t total = nchunks * (uint64_t)MB;
    const uint32_t lead = (uint32_t)((uintptr_t)mask & 3u);          // bytes between the aligned dword below the mask and the mask
    if (4 * t >= total + lead) return;
    const int64_t b0 = (int64_t)(4 * t) - (int64_t)lead;             // the dword's first byte, as an index into the mask
    uint64_t c = b0 > 0 ? (uint64_t)b0 / MB : 0;
    uint32_t j = b0 > 0 ? (uint32_t)((uint64_t)b0 % MB) : 0;
    uint64_t seen = ~0ull;                                           // the chunk whose class, slot and rows are loaded
    uint8_t k = kZoneNone;
    uint32_t rows = 0;
    const uint8_t* src = nullptr;
    uint32_t word = 0;
    uint8_t byte[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t b = b0 + q;
        byte[q] = 0;
        if (b < 0 || (uint64_t)b >= total) continue;
        if (c != seen) {
            seen = c;
            k = cls[c];
            if (k == kZoneDecode) src = cmask + pos[c] * (uint64_t)MB;
            else rows = k == kZoneAll ? zone_rows(zlen[c], chunk_len, D) : 0u;
        }
        byte[q] = k == kZoneDecode ? src[j] : zone_all_mask_byte(rows, j);
        if (++j == MB) { j = 0; c++; }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) word |= (uint32_t)byte[q] << (8 * q);
    if (b0 >= 0 && (uint64_t)b0 + 4 <= total) {
        *(uint32_t*)(mask + b0) = word;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (b0 + q >= 0 && (uint64_t)(b0 + q) < total) mask[b0 + q] = byte[q];
    }
}

int zone_fail(const char* op, const char* what)
{
    const std::string named = std::string(op) + ": " + what;
    return fail(SPRINTZ_E_INVALID, named.c_str());
}

// what the two prune entry points check alike, before the device is touched
int check_prune(const char* op, int elem_bytes, uint32_t chunk_len, uint16_t ndims, const void* d_offsets, const void* d_zmin, const void* d_zmax,
                const void* d_zlen, const void* d_class, const void* d_pos, const void* d_surv_offsets, const void* d_tmp)
{
    if (elem_bytes != 1 && elem_bytes != 2) return zone_fail(op, "elem_bytes must be 1 or 2");
    if (ndims == 0) return zone_fail(op, "ndims == 0");
    if (ndims > 512) return fail(SPRINTZ_E_UNSUPPORTED, "more than 512 columns: no zone map");
    if (chunk_len == 0 || chunk_len > (1u << 30)) return zone_fail(op, "chunk_len must be in 1..2^30");
    if (!d_offsets || !d_zmin || !d_zmax || !d_zlen || !d_class || !d_pos || !d_surv_offsets || !d_tmp) return zone_fail(op, "null device pointer");
    if ((uintptr_t)d_zmin % (uintptr_t)elem_bytes || (uintptr_t)d_zmax % (uintptr_t)elem_bytes) return zone_fail(op, "d_zmin / d_zmax must be aligned to the element size");
    if ((uintptr_t)d_offsets % 8 || (uintptr_t)d_zlen % 8 || (uintptr_t)d_pos % 8 || (uintptr_t)d_surv_offsets % 8 || (uintptr_t)d_tmp % 8)
        return zone_fail(op, "d_offsets, d_zlen, d_pos, d_surv_offsets and d_tmp must be aligned to 8 bytes");
    return 0;
}

// classify -> scan -> compact on one stream
int prune(const char* op, bool linear, int elem_bytes, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint64_t* d_offsets, const void* d_zmin,
          const void* d_zmax, const int64_t* d_zlen, const ZonePredicate& p, uint8_t* d_class, uint64_t* d_pos, uint64_t* d_surv_offsets, void* d_tmp,
          hipStream_t st)
{
    if (!have_device()) return fail(SPRINTZ_E_NO_DEVICE, "no usable HIP device (libsprintz_mi355x has no CPU fallback)");
    int log2G = 0;                                                   // 1 .. 64 lanes a chunk: as many as it has columns
    while (log2G < 6 && (1u << log2G) < ndims) log2G++;
    const uint64_t grid = ((nchunks << log2G) + kThreads - 1) / kThreads, grid2 = (nchunks + 1 + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return zone_fail(op, "too many chunks for one launch");
    uint32_t* flags = (uint32_t*)d_tmp;
    void* scan_tmp = (uint8_t*)d_tmp + zone_flags_bytes(nchunks);
#define SPRINTZ_ZONE_CLASSIFY(T, LIN)                                                                                                          \
    hipLaunchKernelGGL((zone_classify_kernel<T, LIN>), dim3((unsigned)grid), dim3(kThreads), 0, st, nchunks, chunk_len, (uint32_t)ndims, log2G, \
                       d_offsets, (const T*)d_zmin, (const T*)d_zmax, d_zlen, p, d_class, flags)
    if (elem_bytes == 1) {
        if (linear) SPRINTZ_ZONE_CLASSIFY(uint8_t, true);
        else SPRINTZ_ZONE_CLASSIFY(uint8_t, false);
    } else {
        if (linear) SPRINTZ_ZONE_CLASSIFY(uint16_t, true);
        else SPRINTZ_ZONE_CLASSIFY(uint16_t, false);
    }
#undef SPRINTZ_ZONE_CLASSIFY
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_size_scan(flags, nchunks, 1, d_pos, scan_tmp, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(zone_compact_kernel, dim3((unsigned)grid2), dim3(kThreads), 0, st, nchunks, d_offsets, d_class, d_pos, d_surv_offsets);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        const std::string named = std::string(op) + ": a kernel launch failed: " + hipGetErrorString(e);
        return fail(SPRINTZ_E_HIP, named.c_str());
    }
    return 0;
}

}  // namespace
}  // namespace sprintz

using namespace sprintz;

extern "C" {

size_t sprintz_mi355x_zone_prune_tmp_bytes(uint64_t nchunks)
{
    if (nchunks == 0 || nchunks > (1ull << 40)) return 0;
    return zone_flags_bytes(nchunks) + sprintz_mi355x_compact_tmp_bytes(nchunks);
}

int sprintz_mi355x_zone_prune_box(int elem_bytes, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint64_t* d_offsets, const void* d_zmin,
                                  const void* d_zmax, const int64_t* d_zlen, const void* d_lo, const void* d_hi, uint32_t mode, uint8_t* d_class,
                                  uint64_t* d_pos, uint64_t* d_surv_offsets, void* d_tmp, void* hip_stream)
{
    const char* op = "zone_prune_box";
    int rc = check_prune(op, elem_bytes, chunk_len, ndims, d_offsets, d_zmin, d_zmax, d_zlen, d_class, d_pos, d_surv_offsets, d_tmp);
    if (rc) return rc;
    if (mode != SPRINTZ_FILTER_ALL && mode != SPRINTZ_FILTER_ANY) return zone_fail(op, "mode must be SPRINTZ_FILTER_ALL or SPRINTZ_FILTER_ANY");
    if (!d_lo || !d_hi) return zone_fail(op, "null device pointer");
    if ((uintptr_t)d_lo % (uintptr_t)elem_bytes || (uintptr_t)d_hi % (uintptr_t)elem_bytes) return zone_fail(op, "d_lo / d_hi must be aligned to the element size");
    if (nchunks == 0) return 0;
    const ZonePredicate p{d_lo, d_hi, nullptr, mode, 0, 0, 0};
    return prune(op, false, elem_bytes, nchunks, chunk_len, ndims, d_offsets, d_zmin, d_zmax, d_zlen, p, d_class, d_pos, d_surv_offsets, d_tmp, (hipStream_t)hip_stream);
}

int sprintz_mi355x_zone_prune_linear(int elem_bytes, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint64_t* d_offsets, const void* d_zmin,
                                     const void* d_zmax, const int64_t* d_zlen, const int32_t* d_weights, int32_t bias, int32_t lo, int32_t hi,
                                     uint8_t* d_class, uint64_t* d_pos, uint64_t* d_surv_offsets, void* d_tmp, void* hip_stream)
{
    const char* op = "zone_prune_linear";
    int rc = check_prune(op, elem_bytes, chunk_len, ndims, d_offsets, d_zmin, d_zmax, d_zlen, d_class, d_pos, d_surv_offsets, d_tmp);
    if (rc) return rc;
    if (!d_weights) return zone_fail(op, "null device pointer");
    if ((uintptr_t)d_weights % 4) return zone_fail(op, "d_weights must be aligned to 4 bytes");
    if (chunk_len % ndims) return zone_fail(op, "chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if (nchunks == 0) return 0;
    const ZonePredicate p{nullptr, nullptr, d_weights, 0u, bias, lo, hi};
    return prune(op, true, elem_bytes, nchunks, chunk_len, ndims, d_offsets, d_zmin, d_zmax, d_zlen, p, d_class, d_pos, d_surv_offsets, d_tmp, (hipStream_t)hip_stream);
}

int sprintz_mi355x_zone_expand(uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint8_t* d_class, const uint64_t* d_pos, const int64_t* d_zlen,
                               const uint8_t* d_cmask, const uint32_t* d_ccounts, const int64_t* d_crets, uint8_t* d_mask, uint32_t* d_counts,
                               int64_t* d_rets, void* hip_stream)
{
    const char* op = "zone_expand";
    if (ndims == 0) return zone_fail(op, "ndims == 0");
    if (chunk_len == 0 || chunk_len > (1u << 30)) return zone_fail(op, "chunk_len must be in 1..2^30");
    if (!d_class || !d_pos || !d_zlen) return zone_fail(op, "null device pointer");
    if (!d_mask && !d_counts) return zone_fail(op, "neither a mask nor counts asked for");
    if ((uintptr_t)d_pos % 8 || (uintptr_t)d_zlen % 8 || (uintptr_t)d_crets % 8 || (uintptr_t)d_rets % 8)
        return zone_fail(op, "d_pos, d_zlen, d_crets and d_rets must be aligned to 8 bytes");
    if ((uintptr_t)d_ccounts % 4 || (uintptr_t)d_counts % 4) return zone_fail(op, "d_ccounts and d_counts must be aligned to 4 bytes");
    if (nchunks == 0) return 0;
    if (!have_device()) return fail(SPRINTZ_E_NO_DEVICE, "no usable HIP device (libsprintz_mi355x has no CPU fallback)");
    const uint32_t rows = (chunk_len + ndims - 1) / ndims, MB = (rows + 7) / 8;
    const uint64_t dwords = d_mask ? (nchunks * (uint64_t)MB + 3 + 3) / 4 : 0;       // the mask's bytes and up to 3 in front of them
    const uint64_t threads = dwords > nchunks ? dwords : nchunks, grid = (threads + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return zone_fail(op, "too many chunks for one launch");
    hipLaunchKernelGGL(zone_expand_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)hip_stream, nchunks, chunk_len, (uint32_t)ndims, MB, d_class,
                       d_pos, d_zlen, d_cmask, d_ccounts, d_crets, d_mask, d_counts, d_rets);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        const std::string named = std::string(op) + ": kernel launch failed: " + hipGetErrorString(e);
        return fail(SPRINTZ_E_HIP, named.c_str());
    }
    return 0;
}

}  // extern "C"
