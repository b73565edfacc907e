// decode_moments.hip -- the moments-rows instantiations (Q == kQueryMoments) of the generic decoder and of decode_fast, both
// widths, both codecs.  A translation unit of their own, as decode_aggregate.hip: the kernels of decode_w8.hip / decode_w16.hip keep the
// code and the flags they had.  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
namespace sprintz {
hipError_t decode_generic_moments(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryMoments) return hipErrorInvalidValue;
    shmem = 0;                                             // whatever the plan carved: nothing is staged
    if (w == 8) { SPRINTZ_DISPATCH_Q(decode_kernel, 8, kQueryMoments) }
    if (w == 16) { SPRINTZ_DISPATCH_Q(decode_kernel, 16, kQueryMoments) }
    return hipErrorInvalidValue;
}
// reduce only: every mapping the windowed query has
hipError_t decode_fast_moments(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryMoments || ds != 0 || a.col_stride) return hipErrorInvalidValue;
    if (w == 16) { SPRINTZ_DISPATCH_DECODE_FAST_Q(decode_fast_kernel, 16, kQueryMoments, false) }
    if (w == 8) { SPRINTZ_DISPATCH_DECODE_FAST_Q(decode_fast_kernel, 8, kQueryMoments, false) }
    return hipErrorInvalidValue;
}
}  // namespace sprintz
