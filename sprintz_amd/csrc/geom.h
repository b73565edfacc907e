// geom.h -- the shape arithmetic host and kernels share: workgroup size, alignment units, lane mappings, the LDS carves and task
// geometries the kernels take as arguments, the stream bound.  Plain C++17, no HIP: the kernel headers include it for the structs
// their kernels read, plan.h for the decisions it takes from them, and a host compiler builds both (tests/plan_probe.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef SPRINTZ_THREADS
#define SPRINTZ_THREADS 256
#endif
#ifndef SPRINTZ_BOUND_ALIGN
#define SPRINTZ_BOUND_ALIGN 128           // sprintz_mi355x_compress_bound is a multiple of this: slots start on 128-byte lines
#endif
#ifndef SPRINTZ_ENC_DRAIN_ALIGN
#define SPRINTZ_ENC_DRAIN_ALIGN 128       // encode_fast.h / encode_wide.h: granularity of the window's flushes to the slot
#endif

namespace sprintz {

constexpr int kThreads = SPRINTZ_THREADS;        // wavefronts per workgroup x 64

// Q (template parameter of the decoders): 0 = plain decode; 1 = decode + reduce; 2 = reduce only (nothing is written
// to `out` -- QueryParams::materialize == false); 3 = per-window min / max / sum, reduce only;
// 4 = gather: a lane group decodes one PIECE (a range's rows [lo, hi) of one chunk), stores those rows alone and stops after row hi - 1;
// 5 = filter: one bit per row -- does the row satisfy the per-column bounds? -- and the chunk's count of them, reduce only;
// 6 = select: a chunk is decoded once and only the rows whose bit is set in the caller's mask are stored, packed densely behind the chunk's base;
// 7 = aggregate: per-window min / max / sum / count of the rows whose bit is set in the caller's mask, reduce only;
// 8 = histogram: per-column value counts of the rows a mask names (or of every row), counted in an LDS table a workgroup, reduce only;
// 9 = moments: per-window count, sum, sum of squares and sum of products with one reference column of the rows a mask names (or of every row), reduce only;
// 10 = group-by: per bin of ONE key column's value, the count and the per-column sums of the rows a mask names (or of every row), added up in an LDS table a workgroup, reduce only;
// 11 = extrema: per-window min / max with the rows they stand in, the first and the last selected row and the count, of the rows a mask names (or of every row), reduce only;
// 12 = linear filter: one bit per row -- does bias + sum_d w[d] x[g, d] + sum_d u[d] x[g - 1, d], in wrapping 32-bit arithmetic, lie in [lo, hi]? -- and the
// chunk's count of them, in the filter's mask layout, reduce only;
// 13 = segment: per run of rows that a mask names (or per stretch between two set bits) its start, length and min / max / sum, placed behind the chunk's base, reduce only;
// 14 = float: a plain decode whose stores convert -- every sample leaves as fl32(fl32(x * scale[d]) + offset[d]) in float32, float16 or bfloat16, never as an integer;
// 15 = rolling: per element the min / max / sum of its column over the W rows that end at its row (a trailing window, clipped at the chunk's first row
// inside the launch; the seam pass of decode_rolling.hip carries it over the chunk seams), stored at the element's place in place of the element;
// 16 = project: a plain decode (or float rows) that stores only the K columns a slot table names, each at its slot of a dense [rows, K] output;
// 17 = cumulative: per element the running min / max / sum of its column from the batch's first row to its row, stored at the element's place in place of
// the element; a chunk starts from the state the scan of decode_cumulative.hip left for it;
// 18 = derive: nothing of a decoded row is stored but K linear forms of it and of the row in front of it -- the linear filter's sum itself, K times, as int32
// or converted as float rows convert -- each at its place of a dense [rows, K] output; the seam pass of decode_derive.hip carries the lag term over the chunk seams;
// 19 = fir: per element bias[d] + sum_j taps[j][d] x[g - j, d] over the T rows that end at its row -- a per-column tap filter, as int32 or converted as derive
// rows convert -- stored at the element's place; rows in front of the chunk's first contribute nothing inside the launch, and the seam pass of decode_fir.hip
// computes the first T - 1 rows of every chunk again from raw rows.
// 6 .. 11 and 13 read one row mask (decode_ops.h: RowMaskArgs), 3, 7, 9 and 11 walk one set of windows (WindowArgs), 8 and 10 fill one table of bins (BinTableArgs)
constexpr int kQueryOff = 0, kQueryMaterialize = 1, kQueryReduceOnly = 2, kQueryWindow = 3, kQueryGather = 4, kQueryFilter = 5, kQuerySelect = 6,
              kQueryAggregate = 7, kQueryHistogram = 8, kQueryMoments = 9, kQueryGroupBy = 10, kQueryExtrema = 11, kQueryLinear = 12, kQuerySegment = 13, kQueryFloat = 14, kQueryRolling = 15;
constexpr int kQueryProject = 16;
constexpr int kQueryCumulative = 17;
constexpr int kQueryDerive = 18;
constexpr int kQueryFir = 19;
// the modes that never store a decoded sample
constexpr bool query_reduce_only(int q)
{
    return q == kQueryReduceOnly || q == kQueryWindow || q == kQueryFilter || q == kQueryAggregate || q == kQueryHistogram || q == kQueryMoments || q == kQueryGroupBy || q == kQueryExtrema || q == kQueryLinear || q == kQuerySegment;
}
// float rows: the output format (SPRINTZ_FLOAT_F32 / _F16 / _BF16) and the signed bit travel in one word (FilterArgs::mode, decode_ops.h);
// an output element's bytes
constexpr uint32_t kFloatF32 = 0, kFloatF16 = 1, kFloatBF16 = 2, kFloatSignedBit = 4;
constexpr int float_out_bytes(uint32_t mode) { return (mode & 3u) == kFloatF32 ? 4 : 2; }
// project rows: the same word, with one bit more for "the element type, unconverted"; an output element's bytes
constexpr uint32_t kProjectRawBit = 8;
constexpr int project_out_bytes(uint32_t mode, int esz) { return (mode & kProjectRawBit) ? esz : float_out_bytes(mode); }
// derive rows: float rows' word, with one bit more for "the int32 sum, unconverted" (the same bit project rows use for their raw format); an output
// element's bytes; the most forms a call takes
constexpr uint32_t kDeriveI32Bit = 8;
constexpr int derive_out_bytes(uint32_t mode) { return (mode & kDeriveI32Bit) ? 4 : float_out_bytes(mode); }
constexpr uint32_t kDeriveMaxForms = 16;
// rolling rows: the ops (SPRINTZ_ROLL_MIN / _MAX / _SUM, WindowArgs::ops) and the LDS a workgroup's launch can be given.  A chunk's history
// ring holds the last W + 8 raw rows of its columns, column by column (a lane reads 8 rows of a column as one piece), rounded up to 16 bytes
constexpr uint32_t kRollMin = 1, kRollMax = 2, kRollSum = 4;
constexpr uint64_t kRollLdsMax = 160ull * 1024ull;
constexpr uint64_t roll_ring_bytes(uint32_t W, int D, int esz) { return (((uint64_t)W + 8ull) * (uint64_t)D * (uint64_t)esz + 15ull) & ~15ull; }
// the largest window the sum's int32 holds exactly, W (2^(8 esz) - 1) < 2^31, as a multiple of 8
constexpr uint32_t roll_sum_max_window(int esz) { return (uint32_t)(0x7fffffffull / ((1ull << (8 * esz)) - 1ull)) & ~7u; }
// the largest window (a multiple of 8; 0: none) whose rings -- one for each of the `groups` chunks of a workgroup -- fit kRollLdsMax and whose
// sum fits int32: what the planner refuses beyond and what the host wrapper names in its refusal
constexpr uint32_t roll_max_window(int D, int esz, uint32_t groups)
{
    const uint64_t rows = (kRollLdsMax / groups & ~15ull) / ((uint64_t)D * (uint64_t)esz);      // rows of one ring
    const uint64_t w = rows < 16 ? 0 : (rows - 8) & ~7ull;
    return w > roll_sum_max_window(esz) ? roll_sum_max_window(esz) : (uint32_t)w;
}
// with more than one chunk: what one chunk leaves for the seam pass (decode_ops.h: RollSlot) -- a word with the elements the chunk decoded to (0: damaged),
// 12 bytes of padding, then its last W - 1 rows in the element type where it is full; a multiple of 16 bytes
constexpr uint64_t roll_tmp_stride(uint32_t W, int D, int esz) { return (16ull + ((uint64_t)W - 1ull) * (uint64_t)D * (uint64_t)esz + 15ull) & ~15ull; }
// FIR rows: the most taps a call takes; the history a filter of T taps keeps -- rolling rows' ring with W replaced by Wh, T - 1 rounded up to whole blocks
// of 8 rows (roll_ring_bytes(fir_history_rows(T), D, esz)); and what one chunk leaves for the seam pass (decode_ops.h: FirSlot) -- a word with the elements
// the chunk decoded to (0: damaged), 12 bytes of padding, its first T - 1 raw rows, then its last T - 1 raw rows where it is full; a multiple of 16 bytes
constexpr uint32_t kFirMaxTaps = 256;
constexpr uint32_t fir_history_rows(uint32_t T) { return (T + 6u) & ~7u; }
constexpr uint64_t fir_tmp_stride(uint32_t T, int D, int esz) { return (16ull + 2ull * ((uint64_t)T - 1ull) * (uint64_t)D * (uint64_t)esz + 15ull) & ~15ull; }
// the most taps (0: none) whose rings -- one for each of the `groups` chunks of a workgroup -- fit kRollLdsMax
constexpr uint32_t fir_max_taps(int D, int esz, uint32_t groups)
{
    const uint64_t rows = (kRollLdsMax / groups & ~15ull) / ((uint64_t)D * (uint64_t)esz);      // rows of one ring
    const uint64_t t = rows < 8 ? 0 : ((rows - 8) & ~7ull) + 1;
    return t > kFirMaxTaps ? kFirMaxTaps : (uint32_t)t;
}
// cumulative rows: the ops (SPRINTZ_CUM_MIN / _MAX / _SUM, WindowArgs::ops; WindowArgs::count carries sum_bytes) and the scan over the chunks'
// totals (decode_cumulative.hip).  A workgroup of the scan owns one column and walks the chunks kCumScanTile at a step: each of its kThreads
// threads takes kCumScanChunks consecutive chunks.
constexpr uint32_t kCumMin = 1, kCumMax = 2, kCumSum = 4;
constexpr uint32_t kCumScanChunks = 8;
constexpr uint32_t kCumScanTile = (uint32_t)kThreads * kCumScanChunks;
// The call's scratch (sprintz_mi355x_cumulative_tmp_bytes), five regions that each start on 16 bytes: the chunks' entering states -- chunk c's at
// uint64 [c][3][D], a min row, a max row and a sum row, the carries' own layout -- then what the totals pass writes: its return values int64 [n],
// the chunks' sums uint64 [n][D], their minima and their maxima in the element type [n][D] (sized for 2-byte elements)
struct CumTmp { uint64_t state, rets, sum, min, max, bytes; };
constexpr uint64_t cum_round16(uint64_t x) { return (x + 15ull) & ~15ull; }
constexpr CumTmp cum_tmp_layout(uint64_t nchunks, int D)
{
    const uint64_t nd = nchunks * (uint64_t)D;
    const uint64_t rets = cum_round16(nd * 24ull), sum = rets + cum_round16(nchunks * 8ull), mn = sum + cum_round16(nd * 8ull),
                   mx = mn + cum_round16(nd * 2ull);
    return CumTmp{0, rets, sum, mn, mx, mx + cum_round16(nd * 2ull)};
}
// histogram rows: the counters of one call (ndims x nbins; SPRINTZ_HIST_MAX_COUNTERS), 4 bytes each in a workgroup's LDS table, and the
// dynamic LDS a decode_fast.h launch may ask for with its table behind the groups' carves: two such workgroups fit a CU's 160 KB
constexpr uint32_t kHistMaxCounters = 16384;
// group-by rows: the entries of one call's table, nbins x (ndims + 1) (SPRINTZ_GBY_MAX_COUNTERS), under the same LDS budget
constexpr uint32_t kGroupByMaxCounters = 16384;
constexpr uint32_t kHistFastLdsBudget = 80u * 1024u;
// linear filter rows with a lag term: the scratch one chunk leaves for the seam pass (decode_ops.h: LinearSlot) -- a word that says whether the
// chunk has a row, a word of padding, its first and its last existing row in the element type; a multiple of 8 bytes
constexpr uint64_t linear_tmp_stride(int esz, int D) { return (8ull + 2ull * (uint64_t)D * (uint64_t)esz + 7ull) & ~7ull; }

// sprintz_mi355x_compress_bound: the longest stream a chunk of chunk_len elements can have, a multiple of SPRINTZ_BOUND_ALIGN
inline size_t compress_bound(int elem_bytes, uint32_t chunk_len, uint16_t ndims)
{
    const size_t esz = (size_t)elem_bytes, D = ndims ? ndims : 1;
    const size_t hb = elem_bytes == 1 ? 3 : 4;
    const size_t hdr_bytes = (2 * D * hb + 7) / 8;
    const size_t max_groups = chunk_len / (16 * D) + 1;
    // header + per group (header + 2 run bytes worst case beyond raw) + raw payload + flush padding
    const size_t b = 8 + max_groups * (hdr_bytes + 3) + (size_t)chunk_len * esz + 32;
    return (b + (SPRINTZ_BOUND_ALIGN - 1)) & ~(size_t)(SPRINTZ_BOUND_ALIGN - 1);
}

inline bool is_lowdim(int esz, int D) { return esz == 1 ? D <= 4 : D <= 2; }   // sprintz.cpp:34-50

// columns-per-lane values that are instantiated (general layout); low-dim uses CPL = 1
constexpr int kCplSet[] = {1, 2, 3, 4, 5, 6, 8};

struct Mapping { int log2DP; int cpl; };

// Choose lanes-per-chunk (DP = 2^k) and columns-per-lane so that DP*CPL >= D
// with little padding; among mappings within 75% of the best lane utilisation
// prefer the widest group (better coalescing of the D*esz-byte rows).
inline Mapping choose_mapping(int D, bool lowdim)
{
    if (lowdim) {
        int l = 0;
        while ((1 << l) < D) l++;
        return {l, 1};
    }
    double best = 0;
    for (int l = 0; l <= 6; l++)
        for (int c : kCplSet)
            if ((1 << l) * c >= D) best = std::max(best, (double)D / ((1 << l) * c));
    Mapping m{6, 8};
    bool found = false;
    for (int l = 6; l >= 0 && !found; l--) {
        for (int c : kCplSet) {
            if ((1 << l) * c < D) continue;
            if ((double)D / ((1 << l) * c) >= 0.75 * best) { m = {l, c}; found = true; break; }
        }
    }
    return m;
}

// rolling rows: the largest window a SHAPE takes -- roll_max_window at the chunks a workgroup of the generic kernel decodes, kThreads over the
// lanes of its column group (`general`: the general layout asked for, or a codec that has no other).  plan_decode refuses by it and the host
// wrapper names it in its refusal: one function, so that the two cannot drift apart
inline uint32_t roll_shape_max_window(int D, int esz, bool general)
{
    const Mapping m = choose_mapping(D, general ? false : is_lowdim(esz, D));
    return roll_max_window(D, esz, (uint32_t)(kThreads >> m.log2DP));
}

// FIR rows: the most taps a SHAPE takes, by the same rule -- fir_max_taps at the chunks a workgroup of the generic kernel decodes.  plan_decode refuses
// by it and the host wrapper names it in its refusal
inline uint32_t fir_shape_max_taps(int D, int esz, bool general)
{
    const Mapping m = choose_mapping(D, general ? false : is_lowdim(esz, D));
    return fir_max_taps(D, esz, (uint32_t)(kThreads >> m.log2DP));
}

inline uint32_t next_pow2(uint32_t x)
{
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

inline size_t group_bytes_max(int esz, int D)
{
    const size_t hb = esz == 1 ? 3 : 4;
    return (2 * (size_t)D * hb + 7) / 8 + 16 * (size_t)D * esz;
}

// ---- decode_fast.h: bytes of LDS one group needs in decode_fast_kernel
constexpr uint32_t decode_fast_lds_bytes(int W, int DP, int CPL, int D, bool colmajor_burst = false, int DS = 0)
{
    const uint32_t unit = DP * 16 * CPL;
    const uint32_t hb = W == 8 ? 3 : 4;
    const uint32_t dcap = DS ? DS : DP * CPL;
    const uint32_t hdrmax = (2 * dcap * hb + 7) / 8, blkmax = 8 * dcap * (W / 8);
    const uint32_t cg = hdrmax + 2 * blkmax + 4;
    const uint32_t rb = ((2 * (cg + 24) + 3 + unit - 1) / unit + 1) * unit;
    const uint32_t apron = (cg + 24 + 8 + 15) & ~15u;
    // column-major burst staging: 4 blocks of every column the group can hold + 4 row offsets
    const uint32_t stage = colmajor_burst ? 4u * blkmax + 16 : ((8u * D * (W / 8) + 15) & ~15u) + 16;   // +16: spread groups over banks
    return rb + apron + stage;
}

// ---- decode_lat.h
constexpr uint32_t kLatMaxChunkBytes = 16u << 10;     // the stream, the error image and the tables of ONE chunk must fit LDS
constexpr uint32_t lat_align16(uint32_t x) { return (x + 15u) & ~15u; }
// LDS carve: [stream: strm_cap + 32 | grp: NB + 3 pairs of words | err: one int per block element | sum: one word per (column, block)]
struct LatCarve {
    uint32_t strm_cap, o_grp, o_err, o_sum, total;
};
inline LatCarve lat_carve(uint32_t bound_bytes, uint32_t chunk_len, uint32_t D)
{
    LatCarve c;
    const uint32_t nb = chunk_len / (8u * D);
    c.strm_cap = lat_align16(bound_bytes + 32u);
    c.o_grp = c.strm_cap + 32u;
    c.o_err = c.o_grp + lat_align16((nb + 3u) * 8u + 16u);
    c.o_sum = c.o_err + (nb + 1u) * 8u * D * 4u + 16u;      // (+1 block: phase C reads one block ahead)
    c.total = c.o_sum + lat_align16(D * (nb | 1u) * 4u + 16u);
    return c;
}

// ---- encode_lat.h
struct EncLatCarve {
    uint32_t o_dl, o_zz, o_coef, o_nbx, o_rb, o_wo, o_img, img_cap, total;
};
inline EncLatCarve enc_lat_carve(uint32_t bound_bytes, uint32_t chunk_len, uint32_t D, uint32_t esz)
{
    EncLatCarve c;
    const uint32_t nb = chunk_len / (8u * D), body = nb * 8u * D * esz;
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    c.o_dl = al(chunk_len * esz + 16u);
    c.o_zz = c.o_dl + al(body + 16u);
    c.o_coef = c.o_zz + al(body + 16u);
    c.o_nbx = c.o_coef + al(nb * D * 4u + 16u);
    c.o_rb = c.o_nbx + al(nb * D * 4u + 16u);
    c.o_wo = c.o_rb + al(nb * 4u + 16u);
    c.o_img = c.o_wo + al(nb * 8u + 16u);
    c.img_cap = al(bound_bytes + 48u);
    c.total = c.o_img + c.img_cap;
    return c;
}

// ---- decode_row.h
struct RowDecGeom {
    uint32_t U;          // dwords per row = lanes per chunk
    uint32_t G;          // chunks per wavefront = 64 / U
    uint32_t invU;       // ceil(2^16 / U): lane / U == (lane * invU) >> 16 for lane < 64
    uint32_t ok;
};

inline RowDecGeom row_dec_geom(uint32_t esz, uint32_t chunk_len, uint32_t D)
{
    RowDecGeom g{};
    const uint32_t rowbytes = D * esz;
    if (rowbytes % 4u || ((uint64_t)chunk_len * esz) % 4u || chunk_len < 16u * D) return g;
    g.U = rowbytes / 4u;
    if (g.U > 64u) return g;
    g.G = 64u / g.U;
    g.invU = (65536u + g.U - 1u) / g.U;
    g.ok = 1u;
    return g;
}

// ---- decode_blk.h
struct BlkDecGeom {
    uint32_t P, NBC, T, CPW;
    uint32_t img_cap;                                    // bytes of one chunk's stream image (multiple of 16)
    uint32_t o_desc, o_psum, o_csum, o_info, total;      // LDS carve (bytes)
    uint32_t invT, invP;                                 // ceil(2^16 / T), ceil(2^16 / P): n / d == (n * inv) >> 16 for n < 256, d <= 256
    uint32_t ok;
};

inline BlkDecGeom blk_dec_geom(uint32_t esz, uint32_t chunk_len, uint32_t D, uint32_t bound_bytes)
{
    BlkDecGeom g{};
    const uint32_t rowbytes = D * esz, hb = esz == 1 ? 3u : 4u;
    if (rowbytes % 16u || ((uint64_t)chunk_len * esz) % 16u || chunk_len < 32u * D) return g;      // (>= 4 blocks: the scan's lanes are tasks)
    if (2u * D > 16u * (hb == 3u ? 10u : 8u)) return g;  // a group header's 2 D fields over the walk's 16 lanes: 10 x 3 / 8 x 4 bits each (80 / 64 columns)
    g.P = rowbytes / 16u;
    g.NBC = chunk_len / (8u * D);
    g.T = g.NBC * g.P;
    if (g.T > 256u || g.NBC >= 32767u) return g;
    g.img_cap = (bound_bytes + 64u + 15u) & ~15u;        // + the start's phase in its 16-byte piece, + windows that look past the last byte
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    uint32_t cpw = 256u / g.T;
    if (cpw > 16u) cpw = 16u;                            // (four wavefronts walk four chunks each)
    for (; cpw >= 1; cpw--) {
        g.CPW = cpw;
        g.o_desc = cpw * g.img_cap;
        g.o_psum = g.o_desc + al(cpw * g.NBC * 8u);
        g.o_csum = g.o_psum + al(cpw * g.T * 2u);
        g.o_info = g.o_csum + cpw * g.T * 16u;
        g.total = g.o_info + cpw * 16u;
        if (g.total <= 64u * 1024u) break;
    }
    g.invT = (65536u + g.T - 1u) / g.T;
    g.invP = (65536u + g.P - 1u) / g.P;
    g.ok = cpw >= 1 ? 1u : 0u;
    return g;
}

// ---- encode_blk.h
struct BlkEncGeom {
    uint32_t P;          // 16-byte pieces per row
    uint32_t NBC;        // whole blocks of a full chunk
    uint32_t T;          // tasks per chunk = NBC * P (<= 256)
    uint32_t CPW;        // chunks per workgroup
    uint32_t GW;         // lanes per chunk in the walk: 16 / 32 / 64
    uint32_t img_cap;    // bytes of one chunk's stream image (multiple of 16; >= compress_bound + 16)
    uint32_t o_psum, o_rbits, o_wofs, o_info, total;     // LDS carve (bytes)
    uint32_t ok;
};

inline BlkEncGeom blk_enc_geom(uint32_t esz, uint32_t chunk_len, uint32_t D, uint32_t bound_bytes)
{
    BlkEncGeom g{};
    const uint32_t rowbytes = D * esz;
    if (rowbytes % 16u || ((uint64_t)chunk_len * esz) % 16u || chunk_len < 16u * D) return g;
    g.P = rowbytes / 16u;
    g.NBC = chunk_len / (8u * D);
    g.T = g.NBC * g.P;
    if (g.T == 0 || g.T > 256u || g.NBC >= 32767u) return g;
    g.GW = g.NBC > 32u ? 64u : g.NBC > 16u ? 32u : 16u;
    const uint32_t by_tasks = 256u / g.T, by_walk = 4u * (64u / g.GW);
    g.img_cap = (bound_bytes + 16u + 15u) & ~15u;
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    uint32_t cpw = by_tasks < by_walk ? by_tasks : by_walk;
    for (; cpw >= 1; cpw--) {
        g.CPW = cpw;
        g.o_psum = cpw * g.img_cap;
        g.o_rbits = g.o_psum + al(cpw * g.T * 2u);
        g.o_wofs = g.o_rbits + al(cpw * g.NBC * 4u);
        g.o_info = g.o_wofs + al(cpw * g.NBC * 8u);
        g.total = g.o_info + cpw * 16u;
        if (g.total <= 64u * 1024u) break;
    }
    g.ok = cpw >= 1 ? 1u : 0u;
    return g;
}

// the same scheme for univariate streams of the low-dim layout (encode_blk.h, encode_blk_uni_kernel): P = 1, T = tasks a chunk
// (16 bytes of the series each), NBC = blocks a chunk
inline BlkEncGeom blk_enc_uni_geom(uint32_t esz, uint32_t chunk_len, uint32_t bound_bytes)
{
    BlkEncGeom g{};
    if (((uint64_t)chunk_len * esz) % 16u || chunk_len < 16u) return g;
    g.P = 1;
    g.NBC = chunk_len / 8u;
    g.T = chunk_len * esz / 16u;
    if (g.T == 0 || g.T > 256u) return g;
    // (BASELINE config 1, 128 blocks a chunk: 0.565 ms with 64 lanes a chunk in the walk, 0.661 with 16 -- four chunks a walking wavefront, eight
    //  blocks a lane: the walk's price is its passes over a lane's blocks, not its wave-wide scans; the lane-per-chunk kernel takes 0.399)
    g.GW = g.NBC > 32u ? 64u : g.NBC > 16u ? 32u : 16u;
    const uint32_t by_tasks = 256u / g.T, by_walk = 4u * (64u / g.GW);
    g.img_cap = (bound_bytes + 16u + 15u) & ~15u;
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    uint32_t cpw = by_tasks < by_walk ? by_tasks : by_walk;
    for (; cpw >= 1; cpw--) {
        g.CPW = cpw;
        g.o_psum = cpw * g.img_cap;                      // (unused: one column)
        g.o_rbits = g.o_psum;
        g.o_wofs = g.o_rbits + al(cpw * g.NBC * 4u);
        g.o_info = g.o_wofs + al(cpw * g.NBC * 8u);
        g.total = g.o_info + cpw * 16u;
        if (g.total <= 64u * 1024u) break;
    }
    g.ok = cpw >= 1 ? 1u : 0u;
    return g;
}

}  // namespace sprintz
