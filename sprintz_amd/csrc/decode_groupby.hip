// decode_groupby.hip -- the group-by-rows instantiations (Q == kQueryGroupBy) of the generic decoder and of decode_fast, both
// widths, both codecs.  A translation unit of their own, as decode_histogram.hip: the kernels of decode_w8.hip / decode_w16.hip keep the
// code and the flags they had.  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
namespace sprintz {
// shmem is the workgroup's table of sums and counts alone: nothing is staged (plan.h)
hipError_t decode_generic_groupby(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryGroupBy) return hipErrorInvalidValue;
    if (w == 8) { SPRINTZ_DISPATCH_Q(decode_kernel, 8, kQueryGroupBy) }
    if (w == 16) { SPRINTZ_DISPATCH_Q(decode_kernel, 16, kQueryGroupBy) }
    return hipErrorInvalidValue;
}
// reduce only: every mapping the windowed query has; shmem is the groups' carves with the table behind them
hipError_t decode_fast_groupby(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQueryGroupBy || ds != 0 || a.col_stride) return hipErrorInvalidValue;
    if (w == 16) { SPRINTZ_DISPATCH_DECODE_FAST_Q(decode_fast_kernel, 16, kQueryGroupBy, false) }
    if (w == 8) { SPRINTZ_DISPATCH_DECODE_FAST_Q(decode_fast_kernel, 8, kQueryGroupBy, false) }
    return hipErrorInvalidValue;
}
}  // namespace sprintz
