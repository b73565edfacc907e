// decode_linear.hip -- the linear-filter-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and its seam pass.  decode_uni.h is not taught the
// mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(linear, sprintz::kQueryLinear, SPRINTZ_DISPATCH_DECODE_FAST_ROWS)
namespace sprintz {
// The seam pass.  Inside the decode launch a chunk's first row was its own predecessor; its true predecessor is the last row of the
// chunk in front.  A lane per chunk c >= 1 recomputes row 0's predicate both ways from the decode's scratch alone (decode_ops.h:
// LinearSlot) -- where the two differ, bit 0 of the chunk's first mask byte flips and its count moves by one.  Which way the bit stood is
// known from the scratch, not from the mask: a call without a mask gets its counts right all the same.  A chunk without a row, or
// behind one without (a damaged one: rets says so), is left as it is.
template <int W>
__global__ void __launch_bounds__(kThreads) linear_seam_kernel(DecodeArgs a)
{
    const uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x + 1;
    if (c >= a.nchunks) return;
    const uint32_t D = (uint32_t)a.D;
    const LinearSlot<W> cur = linear_slot<W>(a, c, D), prev = linear_slot<W>(a, c - 1, D);
    if (*cur.has == 0 || *prev.has == 0) return;
    const LinearCtx ctx = linear_ctx(a);
    uint32_t self = 0, seam = 0;
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t w = (uint32_t)a.lin.w[d], u = (uint32_t)a.lin.lag[d], x = cur.first[d];
        self += w * x + u * x;
        seam += w * x + u * (uint32_t)prev.last[d];
    }
    const uint32_t was = linear_hit(ctx, self), is = linear_hit(ctx, seam);
    if (was == is) return;
    if (a.filter.mask) a.filter.mask[c * (uint64_t)a.filter.mask_stride] ^= 1u;
    if (a.filter.counts) a.filter.counts[c] += is - was;
}
hipError_t launch_linear_seam(int esz, const DecodeArgs& a, hipStream_t st)
{
    if (a.nchunks < 2) return hipSuccess;
    const uint64_t grid = (a.nchunks - 1 + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    if (esz == 1) hipLaunchKernelGGL(linear_seam_kernel<8>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(linear_seam_kernel<16>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
}  // namespace sprintz
