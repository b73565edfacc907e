// decode_rolling.hip -- the rolling-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and its seam pass: decode_fast for rows of whole 16-byte pieces on its
// one-column-a-lane mappings (8 .. 64 columns), the generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the
// generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(rolling, sprintz::kQueryRolling, SPRINTZ_DISPATCH_DECODE_FAST_PIECES_1)
namespace sprintz {
// The seam pass.  Inside the decode launch a chunk was its own beginning: the windows of its first W - 1 rows stop at its row 0.  Their
// missing rows are the last rows of the chunk in front, which that chunk left in the decode's scratch (decode_ops.h: RollSlot).  A thread
// per (chunk c >= 1, column d) walks r from W - 2 down to 0: row r lacks the predecessor's last W - 1 - r rows, one more a step, so the
// suffix sum / min / max grows by one row and is combined into out[c, r] -- plain loads and stores, one writer an output element.  A chunk
// behind one that is not full (a damaged one: rets says so) is left as it is; of a short or damaged chunk the rows it has are put right.
template <int W>
__global__ void __launch_bounds__(kThreads) rolling_seam_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    const uint32_t D = (uint32_t)a.D;
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t c = t / D + 1;
    const uint32_t d = (uint32_t)(t % D);
    if (c >= a.nchunks) return;
    const RollSlot<W> cur = rolling_slot<W>(a, c), prev = rolling_slot<W>(a, c - 1);
    if (*prev.elems != a.chunk_len) return;
    const uint32_t n = *cur.elems, w = a.win.rows;
    const uint32_t have = n / D + (d < n % D ? 1u : 0u);        // the rows column d has in chunk c
    const uint32_t lim = have < w - 1u ? have : w - 1u;
    if (lim == 0) return;
    const uint64_t base = c * (uint64_t)a.chunk_len + d;
    uint32_t sum = 0, mn = Elem<W>::MASK, mx = 0;
    for (uint32_t r = w - 1u; r-- > 0;) {
        const uint32_t x = prev.rows[(size_t)r * D + d];
        sum += x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        if (r >= lim) continue;
        const uint64_t e = base + (uint64_t)r * D;
        if (a.win.ops & kRollSum) ((uint32_t*)a.win.sum)[e] += sum;
        if (a.win.ops & kRollMin) {
            U* const p = (U*)a.win.min + e;
            if (mn < (uint32_t)*p) *p = (U)mn;
        }
        if (a.win.ops & kRollMax) {
            U* const p = (U*)a.win.max + e;
            if (mx > (uint32_t)*p) *p = (U)mx;
        }
    }
}
hipError_t launch_rolling_seam(int esz, const DecodeArgs& a, hipStream_t st)
{
    if (a.nchunks < 2) return hipSuccess;
    const uint64_t grid = ((a.nchunks - 1) * (uint64_t)a.D + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    if (esz == 1) hipLaunchKernelGGL(rolling_seam_kernel<8>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(rolling_seam_kernel<16>, dim3((unsigned)grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
}  // namespace sprintz
