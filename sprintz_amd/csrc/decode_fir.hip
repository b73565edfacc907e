// decode_fir.hip -- the FIR-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and its seam pass: decode_fast for rows of whole 16-byte pieces on its
// one-column-a-lane mappings (8 .. 64 columns), the generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the
// generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(fir, sprintz::kQueryFir, SPRINTZ_DISPATCH_DECODE_FAST_PIECES_1)
namespace sprintz {
// The seam pass.  Inside the decode launch a chunk was its own beginning: rows in front of its row 0 contributed nothing to its first T - 1 rows.
// A thread per (chunk c, row r < T - 1, column d) computes y[c, r, d] again, WHOLLY, from raw rows alone -- the chunk's own first rows and the last
// rows of the chunk in front, both in the decode's scratch (decode_ops.h: FirSlot); for chunk 0 the caller's `prev` rows or, without them, the
// chunk's row 0 replicated -- and stores it, converted as the decode converts, over what the decode left: plain loads and stores, one writer an
// output element, no thread waits for another.  Computing again, not adding, is what lets the float formats share the path, and it covers a short
// last chunk with fewer than T - 1 rows.  A damaged chunk (rets says so) and a chunk behind one that is not full are left as the launch wrote them.
template <int W>
__global__ void __launch_bounds__(kThreads) fir_seam_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    const uint32_t D = (uint32_t)a.D, T = fir_ntaps(a), h = T - 1u;
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t d = (uint32_t)(t % D), r = (uint32_t)(t / D % h);
    const uint64_t c = t / D / h;
    if (c >= a.nchunks) return;
    const FirSlot<W> cur = fir_slot<W>(a, c);
    const uint32_t n = *cur.elems;
    if (r >= n / D + (d < n % D ? 1u : 0u)) return;             // the rows column d has in chunk c
    const U* before = (const U*)derive_prev(a);                 // [T - 1][D], its last row is the row in front of row 0
    if (c != 0) {
        const FirSlot<W> prev = fir_slot<W>(a, c - 1);
        if (*prev.elems != a.chunk_len) return;
        before = prev.last;
    }
    uint32_t y = fir_bias(a, d);
    for (uint32_t j = 0; j < T; j++) {
        const uint32_t x = j <= r ? (uint32_t)cur.first[(size_t)(r - j) * D + d] : before ? (uint32_t)before[(size_t)(h + r - j) * D + d] : (uint32_t)cur.first[d];
        y += (uint32_t)a.lin.w[(size_t)j * D + d] * x;
    }
    derive_put(a, c * (uint64_t)a.chunk_len + (uint64_t)r * D + d, y, d);
}
hipError_t launch_fir_seam(int esz, const DecodeArgs& a, hipStream_t st)
{
    if (a.win.count < 2 || a.nchunks == 0) return hipSuccess;
    const uint64_t grid = (a.nchunks * (uint64_t)(a.win.count - 1u) * (uint64_t)a.D + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    if (esz == 1) hipLaunchKernelGGL(fir_seam_kernel<8>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(fir_seam_kernel<16>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
}  // namespace sprintz
