// decode_segment.hip -- the segment-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and the kernel that counts a mask's segments.  decode_uni.h is
// not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(segment, sprintz::kQuerySegment, SPRINTZ_DISPATCH_DECODE_FAST_ROWS)
namespace sprintz {
// Mask -> segments a chunk.  filter_row_ids' lane mapping: a group of G = 2^log2G lanes per chunk, the lanes take the chunk's mask dwords in
// turn (G a trip) and count the rows that start a segment under the rule (decode_ops.h: kSegRuns -- a set bit behind a clear one or at row
// 0; kSegSplits -- a set bit, or row 0), the group adds the counts up and one lane stores the sum.  The dwords are read bytewise: chunk * MB
// has any alignment.  Only rows below rows_c -- `rows`, or what lens[chunk] elements hold of them, none for a negative entry -- count: the
// padding bits of the slot's last byte and the rows a short chunk does not hold are not trusted.  The container is never read.
__global__ void __launch_bounds__(kThreads) segment_count_kernel(const uint8_t* mask, uint64_t nchunks, uint32_t rows, uint32_t MB, uint32_t D, uint32_t mode,
                                                                 const int64_t* lens, int log2G, uint32_t* counts)
{
    const int G = 1 << log2G;
    const uint64_t gtid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = (int)(threadIdx.x & (uint32_t)(G - 1));
    const uint64_t chunk = gtid >> log2G;
    if (chunk >= nchunks) return;                          // whole groups leave together
    const uint8_t* const m = mask + chunk * (uint64_t)MB;
    uint32_t rows_c = rows;
    if (lens) {
        const int64_t n = lens[chunk];
        const uint64_t r = n < 0 ? 0 : (uint64_t)n / D;
        rows_c = r < rows ? (uint32_t)r : rows;
    }
    const uint32_t ndw = (rows_c + 31u) >> 5;              // the dwords that hold a row below rows_c: 4 ndw <= MB + 3
    uint32_t c = 0;
    for (uint32_t d = (uint32_t)lane; d < ndw; d += (uint32_t)G) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (4u * d + b < MB) w |= (uint32_t)m[4u * d + b] << (8u * b);
        const uint32_t left = rows_c - 32u * d;            // (d < ndw: at least 1)
        if (left < 32u) w &= (1u << left) - 1u;
        uint32_t starts;
        if (mode == kSegSplits) {
            starts = w | (d == 0 ? 1u : 0u);
        } else {
            const uint32_t prev = d == 0 ? 0u : (uint32_t)m[4u * d - 1u] >> 7;      // row 32 d - 1 is below rows_c
            starts = w & ~((w << 1) | prev);
        }
        c += (uint32_t)__popc(starts);
    }
    c = group_sum(c, G);
    if (lane == 0) counts[chunk] = c;
}
hipError_t launch_segment_count(const uint8_t* mask, uint64_t nchunks, uint32_t rows, uint32_t D, uint32_t mode, const int64_t* lens, uint32_t* counts, hipStream_t st)
{
    const uint32_t MB = (rows + 7u) >> 3, ndw = (MB + 3u) >> 2;
    int log2G = 2;                                         // 4 .. 64 lanes a chunk: as many as it has mask dwords
    while (log2G < 6 && (1u << log2G) < ndw) log2G++;
    const uint64_t grid = ((nchunks << log2G) + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_count_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, mask, nchunks, rows, MB, D, mode, lens, log2G, counts);
    return hipGetLastError();
}
}  // namespace sprintz
