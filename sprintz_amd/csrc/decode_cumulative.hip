// decode_cumulative.hip -- the cumulative-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT) and its scan: decode_fast for rows of whole 16-byte pieces on its
// one-column-a-lane mappings (8 .. 64 columns), the generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the
// generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(cumulative, sprintz::kQueryCumulative, SPRINTZ_DISPATCH_DECODE_FAST_PIECES_1)
namespace sprintz {
// The scan.  The totals pass (the windowed query, one window a chunk) left every chunk's per-column min / max / sum and its return value in the
// call's scratch (geom.h: cum_tmp_layout).  This kernel turns them into each chunk's ENTERING state -- the seeds combined with every chunk in
// front of it, an exclusive scan over the chunks -- in the table the decode launch reads (decode_ops.h: cumulative_enter), and writes carry_out.
// A damaged chunk (return value < 0) counts as the identity.
// A workgroup owns ONE column and walks all the chunks itself, kCumScanTile at a step: each thread takes kCumScanChunks consecutive chunks,
// combines them in registers, the threads' partial results are scanned across the wavefront with shuffles and across the workgroup's wavefronts
// through LDS, and a running carry takes the tile's total to the next step; the next tile's totals are loaded while this one is
// scanned.  No workgroup waits for another: columns are independent.
// The minimum and the maximum are unsigned in the element type, the sum is a 64-bit add (it wraps modulo 2^64).  An op that was not asked for
// has no totals: its row of the table and of carry_out is the seed throughout.
struct CumPart {
    uint32_t mn, mx;
    uint64_t sum;
};
__device__ __forceinline__ CumPart cum_combine(const CumPart& a, const CumPart& b)
{
    return CumPart{b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.sum + b.sum};
}
__device__ __forceinline__ CumPart cum_shfl_up(const CumPart& v, unsigned d)
{
    return CumPart{(uint32_t)__shfl_up((int)v.mn, d, 64), (uint32_t)__shfl_up((int)v.mx, d, 64), (uint64_t)__shfl_up((unsigned long long)v.sum, d, 64)};
}
template <int W>
__global__ void __launch_bounds__(kThreads) cumulative_scan_kernel(uint64_t nchunks, uint32_t D, uint32_t ops, uint8_t* tmp, const uint64_t* carry_in, uint64_t* carry_out)
{
    using U = typename Elem<W>::U;
    constexpr uint32_t MASK = Elem<W>::MASK;
    constexpr int K = (int)kCumScanChunks, NW = kThreads / 64;
    __shared__ CumPart wave_tot[NW];
    const CumTmp lay = cum_tmp_layout(nchunks, (int)D);
    uint64_t* const state = (uint64_t*)(tmp + lay.state);
    const int64_t* const rets = (const int64_t*)(tmp + lay.rets);
    const uint64_t* const tsum = (const uint64_t*)(tmp + lay.sum);
    const U* const tmin = (const U*)(tmp + lay.min);
    const U* const tmax = (const U*)(tmp + lay.max);
    const uint32_t d = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const CumPart ident{MASK, 0u, 0ull};
    CumPart carry = ident;
    if (carry_in) carry = CumPart{(uint32_t)carry_in[d] & MASK, (uint32_t)carry_in[D + d] & MASK, carry_in[2u * D + d]};
    // this thread's chunks of the tile at `base`: a damaged chunk, a chunk past the last and an op that was not asked for are the identity
    auto load = [&](uint64_t base, CumPart (&x)[K]) {
        const uint64_t c0 = base + (uint64_t)tid * K;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint64_t c = c0 + (uint64_t)k;
            x[k] = ident;
            if (c < nchunks && rets[c] >= 0) {
                const uint64_t i = c * D + d;
                if (ops & kCumMin) x[k].mn = tmin[i];
                if (ops & kCumMax) x[k].mx = tmax[i];
                if (ops & kCumSum) x[k].sum = tsum[i];
            }
        }
    };
    CumPart x[K], nx[K];
    if (nchunks) load(0, x);
    for (uint64_t base = 0; base < nchunks; base += kCumScanTile) {
        const uint64_t c0 = base + (uint64_t)tid * K;
        // the next tile's loads are on their way while this one is scanned (they read the totals, the stores below write the states)
        if (base + kCumScanTile < nchunks) load(base + kCumScanTile, nx);
        CumPart agg = ident;
#pragma unroll
        for (int k = 0; k < K; k++) agg = cum_combine(agg, x[k]);
        // inclusive scan across the wavefront, then the wavefronts in front
        CumPart inc = agg;
#pragma unroll
        for (unsigned s = 1; s < 64; s <<= 1) {
            const CumPart up = cum_shfl_up(inc, s);
            if (lane >= s) inc = cum_combine(up, inc);
        }
        CumPart excl = cum_shfl_up(inc, 1);
        if (lane == 0) excl = ident;
        __syncthreads();                                    // (the step before has read wave_tot)
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        CumPart run = carry, total = carry;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            if ((uint32_t)w < wave) run = cum_combine(run, wave_tot[w]);
            total = cum_combine(total, wave_tot[w]);
        }
        run = cum_combine(run, excl);
        // each chunk's entering state, then the chunk itself
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint64_t c = c0 + (uint64_t)k;
            if (c < nchunks) {
                uint64_t* const p = state + c * 3ull * D + d;
                p[0] = run.mn;
                p[D] = run.mx;
                p[2u * D] = run.sum;
            }
            run = cum_combine(run, x[k]);
        }
        carry = total;
        if (base + kCumScanTile < nchunks) {
#pragma unroll
            for (int k = 0; k < K; k++) x[k] = nx[k];
        }
    }
    if (carry_out && tid == 0) {
        carry_out[d] = carry.mn;
        carry_out[D + d] = carry.mx;
        carry_out[2u * D + d] = carry.sum;
    }
}
hipError_t launch_cumulative_scan(int esz, uint64_t nchunks, uint32_t D, uint32_t ops, void* d_tmp, const uint64_t* carry_in, uint64_t* carry_out, hipStream_t st)
{
    if (esz == 1) hipLaunchKernelGGL(cumulative_scan_kernel<8>, dim3(D), dim3(kThreads), 0, st, nchunks, D, ops, (uint8_t*)d_tmp, carry_in, carry_out);
    else hipLaunchKernelGGL(cumulative_scan_kernel<16>, dim3(D), dim3(kThreads), 0, st, nchunks, D, ops, (uint8_t*)d_tmp, carry_in, carry_out);
    return hipGetLastError();
}
}  // namespace sprintz
