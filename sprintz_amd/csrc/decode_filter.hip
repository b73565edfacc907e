// decode_filter.hip -- the filter-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT), decode_uni's instantiations of the mode and the kernel
// that turns a mask into row numbers.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(filter, sprintz::kQueryFilter, SPRINTZ_DISPATCH_DECODE_FAST_ROWS)
namespace sprintz {
#define SPRINTZ_UNI_FILTER_CASE(WV, NDV)                                                                              \
    if (w == WV && nd == NDV) {                                                                                       \
        constexpr int tpb = decode_uni_threads(WV, NDV);                                                              \
        const unsigned g = (unsigned)((a.nchunks + tpb - 1) / tpb);                                                   \
        if (fire) hipLaunchKernelGGL((decode_uni_kernel<WV, true, NDV, kQueryFilter>), dim3(g), dim3(tpb), 0, st, a);  \
        else hipLaunchKernelGGL((decode_uni_kernel<WV, false, NDV, kQueryFilter>), dim3(g), dim3(tpb), 0, st, a);      \
        return hipGetLastError();                                                                                     \
    }
hipError_t decode_uni_filter(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryFilter) return hipErrorInvalidValue;
    SPRINTZ_UNI_FILTER_CASE(8, 1)
    SPRINTZ_UNI_FILTER_CASE(8, 2)
    SPRINTZ_UNI_FILTER_CASE(8, 3)
    SPRINTZ_UNI_FILTER_CASE(8, 4)
    SPRINTZ_UNI_FILTER_CASE(16, 1)
    SPRINTZ_UNI_FILTER_CASE(16, 2)
    return hipErrorInvalidValue;
}
#undef SPRINTZ_UNI_FILTER_CASE

// Mask -> row numbers.  A group of G = 2^log2G lanes per chunk; the lanes take the chunk's mask dwords in turn (G a trip), a scan of
// their popcounts over the group gives each lane the place of its first id behind bases[chunk], and each lane writes its dword's
// rows in ascending order.  The dwords are read bytewise: chunk * MB has any alignment.  Bits of rows >= rows (the slot's last
// byte) are not trusted.  An id whose place is >= capacity is dropped; each entry has one writer.
__global__ void __launch_bounds__(kThreads) filter_row_ids_kernel(const uint8_t* mask, const uint64_t* bases, uint64_t nchunks, uint32_t rows, uint32_t MB,
                                                                  int log2G, uint64_t* ids, uint64_t capacity)
{
    const int G = 1 << log2G;
    const uint64_t gtid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = (int)(threadIdx.x & (uint32_t)(G - 1));
    const uint64_t chunk = gtid >> log2G;
    if (chunk >= nchunks) return;                          // whole groups leave together
    const uint8_t* const m = mask + chunk * (uint64_t)MB;
    uint64_t base = bases[chunk];
    const uint64_t row0 = chunk * (uint64_t)rows;
    const uint32_t ndw = (MB + 3u) >> 2;
    for (uint32_t d0 = 0; d0 < ndw; d0 += (uint32_t)G) {
        const uint32_t d = d0 + (uint32_t)lane;
        uint32_t w = 0;
        if (d < ndw) {
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (4u * d + b < MB) w |= (uint32_t)m[4u * d + b] << (8u * b);
            const uint32_t left = rows - 32u * d;          // (4 d <= MB - 1 and 8 MB <= rows + 7, so 32 d < rows: no wrap)
            if (left < 32u) w &= (1u << left) - 1u;
        }
        uint32_t tot;
        const uint32_t excl = group_excl_scan((uint32_t)__popc(w), lane, G, tot);
        uint64_t p = base + excl;
        while (w) {
            const uint32_t b = (uint32_t)__ffs((int)w) - 1u;
            w &= w - 1u;
            if (p < capacity) ids[p] = row0 + 32u * d + b;
            p++;
        }
        base += tot;
    }
}
hipError_t launch_filter_row_ids(const uint8_t* mask, const uint64_t* bases, uint64_t nchunks, uint32_t rows, uint64_t* ids, uint64_t capacity, hipStream_t st)
{
    const uint32_t MB = (rows + 7u) >> 3, ndw = (MB + 3u) >> 2;
    int log2G = 2;                                         // 4 .. 64 lanes a chunk: as many as it has mask dwords
    while (log2G < 6 && (1u << log2G) < ndw) log2G++;
    const uint64_t grid = ((nchunks << log2G) + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_row_ids_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, mask, bases, nchunks, rows, MB, log2G, ids, capacity);
    return hipGetLastError();
}
}  // namespace sprintz
