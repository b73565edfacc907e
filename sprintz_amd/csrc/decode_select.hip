// decode_select.hip -- the select-rows instantiations (Q = kQuerySelect) of the generic decoder and of decode_fast, both widths,
// both codecs.  A translation unit of their own, as decode_gather.hip and decode_filter.hip: the kernels of decode_w8.hip /
// decode_w16.hip keep the code and the flags they had.  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
namespace sprintz {
hipError_t decode_generic_select(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQuerySelect) return hipErrorInvalidValue;
    shmem = 0;                                             // whatever the plan carved: scalar stores, no LDS transpose
    if (w == 8) { SPRINTZ_DISPATCH_Q(decode_kernel, 8, kQuerySelect) }
    if (w == 16) { SPRINTZ_DISPATCH_Q(decode_kernel, 16, kQuerySelect) }
    return hipErrorInvalidValue;
}
// row-major destination, rows of whole 16-byte store pieces: 16 columns and more, or 8 columns of 16 bits (the gather's set)
hipError_t decode_fast_select(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)
{
    if (q != kQuerySelect || ds != 0 || a.col_stride) return hipErrorInvalidValue;
    if (w == 16) {
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 8, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 16, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 32, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 64, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 64, 2, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 16, 64, 4, kQuerySelect, false)
    }
    if (w == 8) {
        SPRINTZ_FAST_CASE(decode_fast_kernel, 8, 16, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 8, 32, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 8, 64, 1, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 8, 64, 2, kQuerySelect, false)
        SPRINTZ_FAST_CASE(decode_fast_kernel, 8, 64, 4, kQuerySelect, false)
    }
    return hipErrorInvalidValue;
}
}  // namespace sprintz
