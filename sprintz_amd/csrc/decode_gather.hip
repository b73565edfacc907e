// decode_gather.hip -- the gather-rows instantiations (Q = kQueryGather) of the generic decoder and of decode_fast, both
// widths.  A translation unit of their own: the kernels of decode_w8.hip / decode_w16.hip keep the code they had.
#include "launch.h"
namespace sprintz {
hipError_t decode_generic_gather(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryGather) return hipErrorInvalidValue;
    shmem = 0;                                             // whatever the plan carved: scalar stores, no LDS transpose
    if (w == 8) { SPRINTZ_DISPATCH_Q(decode_kernel, 8, kQueryGather) }
    if (w == 16) { SPRINTZ_DISPATCH_Q(decode_kernel, 16, kQueryGather) }
    return hipErrorInvalidValue;
}
// row-major destination, rows of whole 16-byte store pieces: 16 columns and more, or 8 columns of 16 bits
hipError_t decode_fast_gather(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryGather || ds != 0 || a.col_stride) return hipErrorInvalidValue;
    if (w == 16) {
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 8, 1, kQueryGather, false)
        SPRINTZ_DISPATCH_DECODE_FAST_GATHER(decode_fast_kernel, 16)
    }
    if (w == 8) { SPRINTZ_DISPATCH_DECODE_FAST_GATHER(decode_fast_kernel, 8) }
    return hipErrorInvalidValue;
}
}  // namespace sprintz
