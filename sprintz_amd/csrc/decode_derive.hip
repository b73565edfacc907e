// decode_derive.hip -- the derive-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and its seam pass: decode_fast on its one-column-a-lane mappings, the
// generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(derive, sprintz::kQueryDerive, SPRINTZ_DISPATCH_DECODE_FAST_LANES_1)
namespace sprintz {
// The seam pass.  Inside the decode launch a chunk's first row was its own predecessor; its true predecessor is the last row of the chunk in
// front or, for the batch's first chunk, the caller's `prev` row where one is given.  A lane per (chunk, form) computes s[c * R, k] again from
// the decode's scratch alone (decode_ops.h: LinearSlot) and stores it, converted as the decode converts, over what the decode left.  A chunk
// without a row, or behind one without (a damaged one: rets says so), is left as it is; so is chunk 0 without `prev`.
template <int W>
__global__ void __launch_bounds__(kThreads) derive_seam_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    const uint32_t K = derive_k(a), D = (uint32_t)a.D;
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t c = t / K;
    const uint32_t k = (uint32_t)(t % K);
    if (c >= a.nchunks) return;
    const U* const given = (const U*)derive_prev(a);
    if (c == 0 && !given) return;
    const LinearSlot<W> cur = linear_slot<W>(a, c, D);
    if (*cur.has == 0) return;
    const U* before = given;
    if (c != 0) {
        const LinearSlot<W> prev = linear_slot<W>(a, c - 1, D);
        if (*prev.has == 0) return;
        before = prev.last;
    }
    uint32_t s = derive_bias(a, k);
    for (uint32_t d = 0; d < D; d++) s += (uint32_t)a.lin.w[k * D + d] * (uint32_t)cur.first[d] + (uint32_t)a.lin.lag[k * D + d] * (uint32_t)before[d];
    derive_put(a, c * (uint64_t)(a.chunk_len / D) * K + k, s, k);
}
hipError_t launch_derive_seam(int esz, const DecodeArgs& a, hipStream_t st)
{
    const uint64_t grid = (a.nchunks * (uint64_t)a.filter.mask_stride + kThreads - 1) / kThreads;      // (mask_stride: K)
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    if (esz == 1) hipLaunchKernelGGL(derive_seam_kernel<8>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(derive_seam_kernel<16>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
}  // namespace sprintz
