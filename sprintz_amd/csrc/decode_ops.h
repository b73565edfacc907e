// decode_ops.h -- the row operations the decoders carry out while they decode (reduce / window queries, gather, filter, select,
// aggregate, histogram, moments, group-by, extrema, linear filter, segment, float, rolling, project, cumulative and derive rows): each one's arguments, its per-block helpers and its verbatim tail, written once for
// every lane mapping -- and what several of them share, once for all of them: the row mask that names the rows to take (RowMaskArgs,
// run_selected_rows, masked_tail_rows), the walk over a chunk's windows (window_advance, window_tail_rows) and the workgroup's table of
// bins in LDS (BinTableArgs, table_begin .. table_end).  A kernel hands over its lane's columns (`col`, with `genuine` false for a lane
// column past the last one), its place in the group (`lane_d` of `DP` lanes) and the mode's running state; decode_uni.h is the
// lane_d = 0, DP = 1, CPL = D = ND case.  What depends on a kernel's lane mapping -- how a block's rows reach the accumulators, the
// staging and the stores -- stays in that kernel.
#pragma once

#include "sprintz_device.h"

namespace sprintz {

// windowed query (Q == kQueryWindow; sprintz_mi355x_query_windows): chunk c, window w (rows [w*W, (w+1)*W) of the chunk
// slot) and column d land at entry (c*count + w)*D + d of each selected output.  Aggregate and moments rows walk the same windows
// and may count each one's selected rows: chunk c's window w in row_count[c * count + w]
struct WindowArgs {
    uint32_t rows;              // W, a multiple of 8: a block of 8 rows never straddles a window edge (rolling rows: the trailing window's rows)
    uint32_t count;             // windows per chunk slot: ceil(ceil(chunk_len / D) / W) (cumulative rows: sum_bytes, 4 or 8)
    uint32_t ops;               // SPRINTZ_QUERY_WIN_MIN 1 | _MAX 2 | _SUM 4 (rolling rows: SPRINTZ_ROLL_*, cumulative rows: SPRINTZ_CUM_*, the same bits)
    void* min;                  // element type
    void* max;                  // element type
    uint64_t* sum;              // (rolling rows: read as uint32_t*, an entry an element; cumulative rows: an entry an element, uint64 or uint32 by sum_bytes)
    uint32_t* row_count;        // optional (SPRINTZ_AGG_COUNT, SPRINTZ_MOM_COUNT)
};
// gather rows (Q == kQueryGather; sprintz_mi355x_gather_rows): range i is batch rows [starts[i], starts[i] + rows), batch row g
// being row g % rpc of chunk g / rpc; piece slot s = i * pieces + k decodes chunk starts[i] / rpc + k (gather_piece below)
struct GatherArgs {
    const uint64_t* starts;     // [nranges], on the device
    uint64_t nranges;
    uint32_t rows;              // rows of every range
    uint32_t rpc;               // R: rows of a chunk slot, chunk_len / D
    uint32_t pieces;            // P: the most chunks a range can touch, (rows + R - 2) / R + 1
};
// filter rows (Q == kQueryFilter; sprintz_mi355x_filter_rows): row r of chunk c matches if every (mode 0) / some (mode 1) column d
// has lo[d] <= x <= hi[d], unsigned; bit r & 7 of mask[c * mask_stride + (r >> 3)], the chunk's matches in counts[c]
struct FilterArgs {
    const void* lo;             // [D], element type, on the device (float rows: the scale, float32 [D] or null; project rows: of every slot, [K])
    const void* hi;             // (float rows: the offset)
    uint32_t mode;              // SPRINTZ_FILTER_ALL 0 / SPRINTZ_FILTER_ANY 1: wave-uniform, not a template parameter (float rows: format | kFloatSignedBit)
    uint8_t* mask;              // optional (project rows: the slot table, int32 [D]; derive rows: the biases, int32 [K], or null)
    uint32_t* counts;           // optional (derive rows: the caller's `prev` row, [D] of the element type, or null)
    uint32_t mask_stride;       // MB: mask bytes of a chunk slot, ceil(ceil(chunk_len / D) / 8) (project rows: K, the columns of an output row; derive rows: K, the forms)
};
// the rows that select, aggregate, histogram, moments, group-by and extrema rows take: those whose bits are set in chunk c's mask bytes
// mask[c * stride ...] (filter_rows' layout).  mask == null -- where the operation allows it -- is every existing row: a run-time,
// wave-uniform switch, as filter.mode is
struct RowMaskArgs {
    const uint8_t* mask;        // [nchunks][stride]
    uint32_t stride;            // mask bytes of a chunk slot, ceil(rows of a chunk slot / 8)
};
// the table of bins that histogram and group-by rows fill: bin b = ((x - lo) mod 2^W) >> shift of a column's value x takes an add if
// b < nbins, in table c / span_chunks of the outputs.  A workgroup decodes the wg_chunks consecutive chunks from blockIdx.x * wg_chunks
// on and adds them up in its own table of `entries` uint32 at byte table_off of its dynamic LDS -- if they all lie in one table of the
// outputs; if not (or wg_chunks == 0: the planner found that an entry could wrap) every add goes to the outputs directly
struct BinTableArgs {
    uint64_t span_chunks;       // H; 0: the whole batch is one table
    uint32_t shift, nbins;
    uint32_t table_off;         // (rolling rows: where the chunks' history rings start in the launch's LDS)
    uint32_t wg_chunks;
    uint32_t entries;           // histogram: D * nbins counters; group-by: nbins * D sums, then nbins counts
};
// select rows (Q == kQuerySelect; sprintz_mi355x_select_rows): the i-th set bit of chunk c's mask bytes, row r, lands at row
// bases[c] + i of `out` and c * rpc + r at the same place of ids; a place >= capacity is dropped
struct SelectArgs {
    const uint64_t* bases;      // [nchunks]
    uint64_t capacity;          // rows of `out` (and entries of ids)
    uint64_t* ids;              // optional
    uint32_t rpc;               // rows of a chunk slot, chunk_len / D
};
// aggregate rows (Q == kQueryAggregate; sprintz_mi355x_aggregate_rows) is the windowed query over the mask's rows alone: the windows,
// the selected ops, the min / max / sum outputs and the count are WindowArgs', the rows RowMaskArgs'
// histogram rows (Q == kQueryHistogram; sprintz_mi355x_histogram_rows): value x of column d, in a row the mask names, counts in bin b of
// lo[d] (BinTableArgs) of histogram g = c / span_chunks: hist[(g * D + d) * nbins + b]
struct HistogramArgs {
    const void* lo;             // [D], element type, on the device, or null: all zero
    uint64_t* hist;             // [ngroups][D][nbins], zeroed on the stream in front of the launch
};
// moments rows (Q == kQueryMoments; sprintz_mi355x_moments_rows): over the rows the mask names, per chunk-relative window w
// (WindowArgs' rows, count and row_count) and per column d at (c * win.count + w) * D + d, the sum of x_d in win.sum, of x_d^2 in sumsq
// and of x_d * x_ref in cross.  An output that is null is not selected
struct MomentArgs {
    uint64_t* sumsq;            // optional (SPRINTZ_MOM_SUMSQ)
    uint64_t* cross;            // optional (SPRINTZ_MOM_CROSS)
    uint32_t ref;               // the reference column (< D; 0 where cross is null)
};
// group-by rows (Q == kQueryGroupBy; sprintz_mi355x_groupby_rows): a row the mask names whose key column holds x belongs to bin b of
// key_lo (BinTableArgs) of table t = c / span_chunks, and to none if b >= nbins: count[t * nbins + b] takes 1 and
// sum[(t * nbins + b) * D + d] takes x_d, every column d.  An output that is null is not selected
struct GroupByArgs {
    uint64_t* count;            // optional (SPRINTZ_GBY_COUNT): [ntables][nbins], zeroed on the stream in front of the launch
    uint64_t* sum;              // optional (SPRINTZ_GBY_SUM): [ntables][nbins][D], the same
    uint32_t key, key_lo;
};
// extrema rows (Q == kQueryExtrema; sprintz_mi355x_extrema_rows): over the rows the mask names, per chunk-relative window w (WindowArgs'
// rows, count, min, max and row_count) and per column d at (c * win.count + w) * D + d, the minimum and the maximum with the
// chunk-relative row of the FIRST selected row that holds each, and the column's value in the window's first and last selected row; those
// two rows themselves at (c * win.count + w) * 2.  An output that is null is not selected
constexpr uint32_t kExtNoRow = 0xffffffffu;     // SPRINTZ_EXT_NO_ROW: the window has no selected row
struct ExtremaArgs {
    uint32_t* argmin;           // optional (SPRINTZ_EXT_ARGMIN)
    uint32_t* argmax;           // optional (SPRINTZ_EXT_ARGMAX)
    void* first;                // optional (SPRINTZ_EXT_FIRST), element type
    void* last;                 // optional (SPRINTZ_EXT_LAST), element type
    uint32_t* rows;             // optional (SPRINTZ_EXT_ROWS): [.. ][2]
};
// linear filter rows (Q == kQueryLinear; sprintz_mi355x_filter_linear): batch row g matches if lo <= s(g) <= hi, signed, with
// s(g) = bias + sum_d w[d] x[g, d] + sum_d lag[d] x[p(g), d] in wrapping 32-bit arithmetic, x the unsigned element, p(g) = g - 1 and
// p(0) = 0.  The mask, the counts and the mask's stride travel in FilterArgs (filter.mask, filter.counts, filter.mask_stride; its lo / hi
// null), as aggregate rows reuses WindowArgs.  Inside the decode launch a chunk's first row is its own predecessor; with lag given the
// decode leaves every chunk's first and last existing row in tmp (LinearSlot) and the seam pass puts row 0 of the chunks behind the first right
struct LinearArgs {
    const int32_t* w;           // [D], on the device (cumulative rows: the caller's carry_out, uint64 [3][D], in a call of one chunk; else null)
    const int32_t* lag;         // [D], or null: no lag term (derive rows: w and lag are [K][D])
    void* tmp;                  // nchunks x linear_tmp_stride (geom.h) bytes where lag is given (rolling rows: nchunks x roll_tmp_stride, or null with one chunk; cumulative rows: the chunks' entering states, uint64 [nchunks][3][D], or null)
    int32_t lo, hi, bias;
    uint32_t pad;
};

struct DecodeArgs {
    const uint8_t* comp;        // compressed bytes
    const uint64_t* offsets;    // [nchunks] byte offset of each chunk stream
    uint64_t nchunks;
    uint32_t chunk_len;         // elements per decoded chunk slot (output stride)
    int D;                      // ndims
    int log2DP;                 // lanes per chunk = 1 << log2DP
    void* out;                  // decoded elements, chunk c at out + c*chunk_len
    int64_t* rets;              // optional per-chunk element counts
    int vec_store;              // 1: LDS-transposed 16-byte stores are legal (alignment checked on host)
    uint32_t lds_group_stride;  // bytes of LDS per group when vec_store
    // headerless form (sprintz_xff.h:56-58)
    int noheader;
    uint32_t nh_ngroups;
    uint32_t nh_remaining;
    uint32_t chunks_per_group;  // decode_fast: consecutive chunks decoded by one lane group
    // column-major destination (BASELINE config 5): element (row r, column d) at out[d*col_stride + r];
    // chunk c holds rows [c*chunk_len/D, ...).  0 = row-major.
    uint64_t col_stride;
    // non-RLE codecs (sprintz_delta.cpp:64-1391; generic kernel only): 6-byte header {u32 len; u16 ndims},
    // len/(16 D) groups, an all-zero block has no payload and no run length; raw: bit-packing only
    int norle;
    int raw;
    int quirk;                  // 1: replay the runs of 16-bit general-layout FIRE streams as the REFERENCE DECODER does (fire_coef_ref_run16)
    // query-on-compressed (sprintz_delta.h:95-98, sprintz_xff.h:90-93, query.hpp:23-29): kernels
    // instantiated with Q == kQueryMaterialize / kQueryReduceOnly reduce every column of every chunk while decoding
    int qop;                    // 1: max, 2: sum (what lands in qres)
    uint64_t* qres;             // [nchunks][D] per-chunk, per-column partial results
    // a single call on the caller thread's mapped host buffer (decode_lat.h alone): offsets == null -> the one chunk's stream is
    // comp[one_off0, one_off1); host_flag != null -> the kernel ends by writing host_ticket there, after every lane's stores
    uint64_t one_off0, one_off1;
    uint64_t* host_flag;
    uint64_t host_ticket;
    // the row operations, behind everything above so that no field there moves.  hipcc's code for the kernels that read nothing of this
    // block -- the plain decode, the reduce queries -- and for gather and filter still follows where the block's fields lie and how long
    // the struct is: tools/kernel_diff.py shows their register choices and schedules moving when gather and filter shift by anything
    // but a multiple of 64 bytes, or when sizeof(DecodeArgs) changes.  So the two stay put modulo 64 (the windows' and the table's
    // arguments in front of them), and the struct keeps the length it has had since group-by rows: those kernels keep their code.
    // (Extrema rows' arguments came out of keep_size: 40 of its 80 spare bytes, behind every field that was there.  The linear filter's took the
    //  other 40: the spare bytes are used up, and the next mode's arguments have to share a struct that is here, as the linear filter shares
    //  FilterArgs, or move the kernels named above.  Float rows do: scale, offset and format ride in FilterArgs' lo, hi and mode.  Rolling rows
    //  do: WindowArgs, LinearArgs::tmp and BinTableArgs::table_off.  Cumulative rows do: WindowArgs, LinearArgs::tmp and LinearArgs::w.  Derive rows
    //  do: the [K][D] weight tables and the seam scratch in LinearArgs' w, lag and tmp; scale, offset, format, biases, `prev` and K in FilterArgs' lo,
    //  hi, mode, mask, counts and mask_stride; decode_fast.h's table of weights in LDS at BinTableArgs::table_off.)
    WindowArgs win;
    MomentArgs mom;
    BinTableArgs table;
    GatherArgs gather;
    FilterArgs filter;
    SelectArgs select;
    RowMaskArgs rows;
    HistogramArgs hist;
    GroupByArgs gby;
    ExtremaArgs ext;
    LinearArgs lin;
};
static_assert(sizeof(DecodeArgs) == 496 && offsetof(DecodeArgs, gather) % 64 == 184 % 64 && offsetof(DecodeArgs, ext) == 416 && sizeof(ExtremaArgs) == 40 &&
                  offsetof(DecodeArgs, lin) == 456 && sizeof(LinearArgs) == 40,
              "see the row operations' block");

// the verbatim tail starts at any byte: element e of it, one 1- or 2-byte load
typedef uint16_t __attribute__((aligned(1), may_alias)) u16_unaligned;
template <int W> __device__ __forceinline__ uint32_t tail_elem(const uint8_t* t, uint32_t e)
{
    return W == 8 ? (uint32_t)t[e] : (uint32_t)*(const u16_unaligned*)(t + 2 * e);
}

// ---- reduce (Q == kQueryMaterialize / kQueryReduceOnly).  The verbatim tail continues the row-major order: element e sits in
// column e % D.  Each genuine column's maximum and sum take the tail's elements in, then the chunk's result leaves.
template <int W, int CPL>
__device__ __forceinline__ void reduce_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, const int (&col)[CPL],
                                            const bool (&genuine)[CPL], uint32_t (&qmax)[CPL], uint64_t (&qsum)[CPL])
{
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        for (uint32_t e = (uint32_t)col[k]; e < remaining; e += D) {
            const uint32_t x = tail_elem<W>(t, e);
            qmax[k] = x > qmax[k] ? x : qmax[k];
            qsum[k] += x;
        }
        if (a.qres) a.qres[chunk * (uint64_t)D + (uint64_t)col[k]] = a.qop == 1 ? (uint64_t)qmax[k] : qsum[k];
    }
}

// ---- windowed query: one column's entries of one window leave (each entry has exactly one writer -- no atomics), and the
// accumulators start over from the identities (min = all ones, max = 0, sum = 0)
template <int W>
__device__ __forceinline__ void win_flush(const DecodeArgs& a, uint64_t idx, uint32_t& qmin, uint32_t& qmax, uint64_t& qsum)
{
    using U = typename Elem<W>::U;
    if (a.win.ops & 1u) ((U*)a.win.min)[idx] = (U)qmin;
    if (a.win.ops & 2u) ((U*)a.win.max)[idx] = (U)qmax;
    if (a.win.ops & 4u) a.win.sum[idx] = qsum;
    qmin = Elem<W>::MASK;
    qmax = 0;
    qsum = 0;
}
// The verbatim tail, column by column: element e is in column e % D, one row further on than the column's previous one, so a window
// edge can fall inside the tail.  Window `wi` of the chunk (the first of them at entry `wbase`) still takes `wleft` rows.  Then the
// partial window leaves, and the identities of the slot's windows past the data.
template <int W, int CPL>
__device__ __forceinline__ void window_tail(const DecodeArgs& a, const uint8_t* t, uint32_t remaining, uint32_t D, const int (&col)[CPL], const bool (&genuine)[CPL],
                                            uint64_t wbase, uint32_t wi, uint32_t wleft, uint32_t (&qmin)[CPL], uint32_t (&qmax)[CPL], uint64_t (&qsum)[CPL])
{
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        uint32_t w = wi, left = wleft;
        for (uint32_t e = (uint32_t)col[k]; e < remaining; e += D) {
            if (left == 0) {
                win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)col[k], qmin[k], qmax[k], qsum[k]);
                w++;
                left = a.win.rows;
            }
            left--;
            const uint32_t x = tail_elem<W>(t, e);
            qmin[k] = x < qmin[k] ? x : qmin[k];
            qmax[k] = x > qmax[k] ? x : qmax[k];
            qsum[k] += x;
        }
        for (; w < a.win.count; w++) win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)col[k], qmin[k], qmax[k], qsum[k]);
    }
}

// ---- the windows' walk, shared by the windowed query, aggregate rows and moments rows.
// one window's count of selected rows leaves with the window's other entries (one lane of the group: one writer an entry), and starts over
__device__ __forceinline__ void window_count_flush(const DecodeArgs& a, uint64_t widx, uint32_t& cnt, int lane_d)
{
    if (a.win.row_count && lane_d == 0) a.win.row_count[widx] = cnt;
    cnt = 0;
}
// Window `wi` of the chunk (the first of them at entry `wbase`) still takes `wleft` rows, and `n` of them -- a block's 8, a delta run's
// share, a row of the tail; never more than wleft -- are done.  If they complete the window it leaves: flush_cols(w) stores this lane's
// columns' entries of window entry w and starts their accumulators over, the count follows where the mode has one (COUNT), and the
// next window begins.
template <bool COUNT, typename F>
__device__ __forceinline__ void window_advance(const DecodeArgs& a, uint32_t n, uint64_t wbase, uint32_t& wi, uint32_t& wleft, uint32_t& cnt, int lane_d,
                                               F flush_cols)
{
    wleft -= n;
    if (wleft == 0) {
        flush_cols(wbase + wi);
        if constexpr (COUNT) window_count_flush(a, wbase + wi, cnt, lane_d);
        wi++;
        wleft = a.win.rows;
    }
}

// ---- the row mask.  The selected rows among the 8 * nblocks that a delta run repeats from block first_block of the chunk on: the set
// bits of those mask bytes, spread over the group's lanes and summed -- or all of them where mask_bytes (the chunk's) is null.  EVERY
// lane of the group must come here: the sum is a group reduction.  (The bytes lie inside the chunk's: the callers check that the run
// fits the chunk slot.)
__device__ __forceinline__ uint32_t run_selected_rows(const uint8_t* mask_bytes, uint32_t first_block, uint32_t nblocks, int lane_d, int DP)
{
    if (!mask_bytes) return 8u * nblocks;
    uint32_t c = 0;
    for (uint32_t j = (uint32_t)lane_d; j < nblocks; j += (uint32_t)DP) c += (uint32_t)__popc((uint32_t)mask_bytes[first_block + j]);
    return group_sum(c, DP);
}
// The verbatim tail of the masked modes: `nfull` whole rows, row-major from chunk row `row0` (a multiple of 8: the rows of the blocks in
// front).  A partial last row is not a row, and a mask bit of a row the tail does not hold is not read.  mask_at(b) is the chunk's mask
// byte b, asked only where the chunk has one (`masked`).  row(r, on) sees every whole row r of the tail, `on`: the mask names it.
template <typename M, typename R>
__device__ __forceinline__ void masked_tail_rows(uint32_t nfull, uint32_t row0, bool masked, M mask_at, R row)
{
    uint32_t m = 0xffu;
    for (uint32_t r = 0; r < nfull; r++) {
        if ((r & 7u) == 0 && masked) m = mask_at((row0 + r) >> 3);
        row(r, ((m >> (r & 7u)) & 1u) != 0);
    }
}
// The same walk for the windowed modes: a window edge can fall inside the tail, so every row moves the chunk's window on
// (window_advance); the selected ones are counted and go to row(r).  Then the partial window leaves, and the identities of the slot's
// windows past the data.
template <typename M, typename F, typename R>
__device__ __forceinline__ void window_tail_rows(const DecodeArgs& a, uint32_t nfull, uint32_t row0, bool masked, M mask_at, uint64_t wbase, uint32_t wi,
                                                 uint32_t wleft, uint32_t cnt, int lane_d, F flush_cols, R row)
{
    masked_tail_rows(nfull, row0, masked, mask_at, [&](uint32_t r, bool on) {
        if (on) {
            cnt++;
            row(r);
        }
        window_advance<true>(a, 1u, wbase, wi, wleft, cnt, lane_d, flush_cols);
    });
    for (; wi < a.win.count; wi++) {
        flush_cols(wbase + wi);
        window_count_flush(a, wbase + wi, cnt, lane_d);
    }
}

// ---- aggregate rows: the windowed query's accumulators take a row only where its mask bit is set.  For a selected row `am` is all
// ones and `om` is 0, for any other row the other way round: x & am is 0 in front of max and sum, x | om is all ones in front of
// min -- the identities.  x may carry garbage above bit W: max and sum take the element through the AND with Elem<W>::MASK folded into
// am, the minimum selects it with SDWA as the windowed query does.
struct AggregateSel { uint32_t am, om; };
template <int W> __device__ __forceinline__ AggregateSel aggregate_sel(uint32_t m, int row)
{
    const bool on = (m >> row) & 1u;
    return AggregateSel{on ? Elem<W>::MASK : 0u, on ? 0u : 0xffffffffu};
}
template <int W>
__device__ __forceinline__ void aggregate_row(uint32_t x, const AggregateSel& s, uint32_t& qmin, uint32_t& qmax, uint32_t& qbs)
{
    const uint32_t t = x & s.am;
    const uint32_t u = x | s.om;
    qmax = t > qmax ? t : qmax;
    qbs += t;
    if constexpr (W == 16)
        asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(qmin) : "v"(qmin), "v"(u));
    else
        asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(qmin) : "v"(qmin), "v"(u));
}
// The verbatim tail (window_tail_rows): a selected row's elements reach the accumulators of the lane's genuine columns
template <int W, int CPL, typename F>
__device__ __forceinline__ void aggregate_tail(const DecodeArgs& a, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0, const int (&col)[CPL],
                                               const bool (&genuine)[CPL], uint64_t wbase, uint32_t wi, uint32_t wleft, uint32_t (&qmin)[CPL],
                                               uint32_t (&qmax)[CPL], uint64_t (&qsum)[CPL], uint32_t acnt, int lane_d, F mask_at)
{
    auto flush_cols = [&](uint64_t w) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) win_flush<W>(a, w * (uint64_t)D + (uint64_t)col[k], qmin[k], qmax[k], qsum[k]);
    };
    window_tail_rows(a, remaining / D, row0, true, mask_at, wbase, wi, wleft, acnt, lane_d, flush_cols, [&](uint32_t r) {
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
            const uint32_t x = tail_elem<W>(t, r * D + (uint32_t)col[k]);
            qmin[k] = x < qmin[k] ? x : qmin[k];
            qmax[k] = x > qmax[k] ? x : qmax[k];
            qsum[k] += x;
        }
    });
}

// ---- histogram rows.  A sample's test is filter_hit's shape: one masked subtract, one shift, one compare.  The counters are a table in
// the workgroup's LDS (non-returning ds_add_u32; BinTable::tab) or, for a workgroup whose chunks lie in more than one histogram, the
// caller's 64-bit entries themselves (HistCtx::g: the histogram of the chunk being decoded).
#ifndef SPRINTZ_HIST_MERGE
// what a column's 8 rows of one block cost in atomics, all three forms measured in profiles/histogram_rows.txt -- 2 (kept): one add of 8
// where all 8 rows are selected and share a bin, an add a sample otherwise; 1: every run of equal consecutive bins is one add of its
// length; 0: an add a sample
#define SPRINTZ_HIST_MERGE 2
#endif
// ---- the workgroup's table of bins (BinTableArgs), the histogram's and group-by's alike
typedef __attribute__((address_space(3))) uint32_t table_lds_u32;
struct BinTable {
    table_lds_u32* tab;         // the workgroup's table, or null: every add goes to the outputs
    uint32_t shift, nbins;
};
// the table of the outputs that `chunk` belongs to
__device__ __forceinline__ uint64_t table_of_chunk(const DecodeArgs& a, uint64_t chunk) { return a.table.span_chunks ? chunk / a.table.span_chunks : 0; }
// v to entry idx of the workgroup's table (the planner's rule keeps every entry below 2^32), or to the output's entry g[gidx] (all 64 bits)
__device__ __forceinline__ void table_add(const BinTable& t, uint32_t idx, uint64_t* g, uint32_t gidx, uint64_t v)
{
    if (t.tab) (void)__hip_atomic_fetch_add(t.tab + idx, (uint32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(g + gidx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// At the kernel's start, every lane of the workgroup: does the workgroup add in its table?  (Workgroup-uniform: its chunks
// [blockIdx.x * wg_chunks, + wg_chunks) -- those that exist -- lie in one table of the outputs.)  The table is zeroed, behind a barrier.
__device__ __forceinline__ BinTable table_begin(const DecodeArgs& a, uint8_t* smem)
{
    BinTable t{nullptr, a.table.shift, a.table.nbins};
    const uint64_t first = (uint64_t)blockIdx.x * a.table.wg_chunks;
    if (a.table.wg_chunks == 0 || first >= a.nchunks) return t;
    const uint64_t last = (first + a.table.wg_chunks < a.nchunks ? first + a.table.wg_chunks : a.nchunks) - 1;
    if (table_of_chunk(a, first) != table_of_chunk(a, last)) return t;
    t.tab = (table_lds_u32*)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + a.table.table_off);
    for (uint32_t i = threadIdx.x; i < a.table.entries; i += kThreads) t.tab[i] = 0;
    __syncthreads();
    return t;
}
// At the kernel's end, every lane of the workgroup (none has left): behind a barrier the table's nonzero entries are added to the
// outputs, spread over all lanes -- device-scope 64-bit adds: integer sums, exact in any order.  The first n0 entries go to dst0, the
// rest to dst1: the places in the outputs of the workgroup's table (table_of_chunk of its first chunk); one that is null is not selected.
__device__ __forceinline__ void table_end(const DecodeArgs& a, const BinTable& t, uint64_t* dst0, uint32_t n0, uint64_t* dst1)
{
    if (!t.tab) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.table.entries; i += kThreads) {
        uint64_t* const dst = i < n0 ? dst0 : dst1;
        const uint32_t v = t.tab[i];
        if (v != 0 && dst) (void)__hip_atomic_fetch_add(dst + (i < n0 ? i : i - n0), (uint64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the histogram's counters: the workgroup's table or the caller's 64-bit entries themselves (g: the histogram of the chunk being decoded)
struct HistCtx {
    BinTable bin;
    uint64_t* g;
};
struct HistCol { uint32_t lo, base; };    // the column's lo and the index of its bin 0 inside a histogram, column * nbins
template <int W>
__device__ __forceinline__ HistCol hist_col(const DecodeArgs& a, int col, bool genuine)
{
    using U = typename Elem<W>::U;
    return HistCol{genuine && a.hist.lo ? (uint32_t)((const U*)a.hist.lo)[col] : 0u, (uint32_t)col * a.table.nbins};
}
__device__ __forceinline__ uint64_t* hist_of_chunk(const DecodeArgs& a, uint64_t chunk) { return a.hist.hist + table_of_chunk(a, chunk) * a.table.entries; }
__device__ __forceinline__ void hist_add(const HistCtx& c, uint32_t idx, uint32_t n) { table_add(c.bin, idx, c.g, idx, n); }
// (x may carry garbage above bit W: only its low W bits reach the masked difference)
template <int W> __device__ __forceinline__ uint32_t hist_bin(const BinTable& t, const HistCol& h, uint32_t x) { return ((x - h.lo) & Elem<W>::MASK) >> t.shift; }
// one value that `n` selected rows hold (a delta run's constant row, a row of the tail)
template <int W> __device__ __forceinline__ void hist_value(const HistCtx& c, const HistCol& h, uint32_t x, uint32_t n)
{
    const uint32_t b = hist_bin<W>(c.bin, h, x);
    if (b < c.bin.nbins && n != 0) hist_add(c, h.base + b, n);
}
// a column's 8 rows of one block; bit i of m: row i is selected
template <int W>
__device__ __forceinline__ void hist_rows8(const HistCtx& c, const HistCol& h, const uint32_t (&x)[8], uint32_t m)
{
#if SPRINTZ_HIST_MERGE == 1
    uint32_t pb = 0, pc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t b = hist_bin<W>(c.bin, h, x[i]);
        const bool on = b < c.bin.nbins && ((m >> i) & 1u);
        if (on && pc != 0 && b == pb) {
            pc++;
        } else {
            if (pc != 0) hist_add(c, h.base + pb, pc);
            pb = b;
            pc = on ? 1u : 0u;
        }
    }
    if (pc != 0) hist_add(c, h.base + pb, pc);
#else
    uint32_t b[8], diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        b[i] = hist_bin<W>(c.bin, h, x[i]);
        diff |= b[i] ^ b[0];
    }
    if (SPRINTZ_HIST_MERGE == 2 && diff == 0 && m == 0xffu) {     // 2: only a block whose 8 rows are selected and share a bin is one add
        if (b[0] < c.bin.nbins) hist_add(c, h.base + b[0], 8u);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (b[i] < c.bin.nbins && ((m >> i) & 1u)) hist_add(c, h.base + b[i], 1u);
#endif
}
// the workgroup's table holds its histogram's D * nbins counters (table_begin .. table_end)
__device__ __forceinline__ HistCtx hist_begin(const DecodeArgs& a, uint8_t* smem) { return HistCtx{table_begin(a, smem), a.hist.hist}; }
__device__ __forceinline__ void hist_end(const DecodeArgs& a, const HistCtx& c)
{
    table_end(a, c.bin, hist_of_chunk(a, (uint64_t)blockIdx.x * a.table.wg_chunks), a.table.entries, nullptr);
}
// The verbatim tail (masked_tail_rows): a selected row's elements are counted, a column each
template <int W, int CPL, typename F>
__device__ __forceinline__ void hist_tail(const DecodeArgs& a, const HistCtx& c, const HistCol (&h)[CPL], const uint8_t* t, uint32_t remaining, uint32_t D,
                                          uint32_t row0, const int (&col)[CPL], const bool (&genuine)[CPL], F mask_at)
{
    masked_tail_rows(remaining / D, row0, a.rows.mask != nullptr, mask_at, [&](uint32_t r, bool on) {
        if (!on) return;
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) hist_value<W>(c, h[k], tail_elem<W>(t, r * D + (uint32_t)col[k]), 1u);
    });
}

// ---- moments rows.  Every value is an exact unsigned integer: a factor is below 2^16, so a product is below 2^32; a chunk slot has
// fewer than 2^30 rows, so every sum of a chunk is below 2^62.  A lane keeps three 64-bit accumulators a column.
struct MomentAcc { uint64_t sum, sumsq, cross; };
// the reference column's 8 rows of a block, in every lane of the group: column lane * CPL + k lives in slot k of lane `lane`, so lane
// ref / CPL hands over its slot ref % CPL.  at(k, i) is this lane's row i of slot k (garbage above bit W allowed); EVERY lane of the
// group must come here -- a lane whose columns are all past the last one too.  (The slot is picked with wave-uniform AND masks: a
// chain of selects on the slot number is turned into an indexed read of a copy of the rows in scratch memory.)
template <int W, int CPL, typename F>
__device__ __forceinline__ void moments_ref_rows(uint32_t ref, int DP, F at, uint32_t (&xr)[8])
{
    const uint32_t slot = ref % (uint32_t)CPL;
    const int lane = (int)(ref / (uint32_t)CPL);
    uint32_t pick[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) pick[k] = slot == (uint32_t)k ? Elem<W>::MASK : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t mine = at(0, i) & pick[0];
#pragma unroll
        for (int k = 1; k < CPL; k++) mine |= at(k, i) & pick[k];
        xr[i] = (uint32_t)__shfl((int)mine, lane, DP);
    }
}
// one value of the reference column, the same way (a delta run's constant row)
template <int W, int CPL>
__device__ __forceinline__ uint32_t moments_ref_value(uint32_t ref, int DP, const uint32_t (&pv)[CPL])
{
    const uint32_t slot = ref % (uint32_t)CPL;
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) mine |= pv[k] & (slot == (uint32_t)k ? Elem<W>::MASK : 0u);
    return (uint32_t)__shfl((int)mine, (int)(ref / (uint32_t)CPL), DP);
}
// a column's 8 rows of one block; bit i of m: row i is selected.  x(i) may carry garbage above bit W, xr is clean; `cross` is
// wave-uniform (is the output selected?)
template <int W, typename F>
__device__ __forceinline__ void moments_rows8(MomentAcc& acc, F x, const uint32_t (&xr)[8], uint32_t m, bool cross)
{
    uint32_t t[8], bs = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        t[i] = x(i) & (((m >> i) & 1u) ? Elem<W>::MASK : 0u);
        bs += t[i];
    }
    acc.sum += bs;
    if constexpr (W == 8) {
        uint32_t bq = 0, bx = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) bq += t[i] * t[i];
        acc.sumsq += bq;
        if (cross) {
#pragma unroll
            for (int i = 0; i < 8; i++) bx += t[i] * xr[i];
            acc.cross += bx;
        }
    } else {
        // (each product is one 64-bit multiply-add, v_mad_u64_u32; profiles/moments_rows.txt has what else was tried)
#pragma unroll
        for (int i = 0; i < 8; i++) acc.sumsq += (uint64_t)t[i] * t[i];
        if (cross) {
#pragma unroll
            for (int i = 0; i < 8; i++) acc.cross += (uint64_t)t[i] * xr[i];
        }
    }
}
// one value x that `c` selected rows hold, beside the reference column's xr (a delta run's constant row: c < 2^30; a row of the tail)
__device__ __forceinline__ void moments_value(MomentAcc& acc, uint32_t x, uint32_t xr, uint32_t c)
{
    acc.sum += (uint64_t)x * c;
    acc.sumsq += (uint64_t)(x * x) * c;
    acc.cross += (uint64_t)(x * xr) * c;
}
// one column's entries of one window leave (each entry has exactly one writer -- no atomics), and the accumulators start over from 0
__device__ __forceinline__ void moments_flush(const DecodeArgs& a, uint64_t idx, MomentAcc& acc)
{
    if (a.win.sum) a.win.sum[idx] = acc.sum;
    if (a.mom.sumsq) a.mom.sumsq[idx] = acc.sumsq;
    if (a.mom.cross) a.mom.cross[idx] = acc.cross;
    acc = MomentAcc{0, 0, 0};
}
// The verbatim tail (window_tail_rows): a selected row's elements reach the sums of the lane's genuine columns.  The reference column's
// element is read from the tail itself: no lane needs another's.
template <int W, int CPL, typename F>
__device__ __forceinline__ void moments_tail(const DecodeArgs& a, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0, const int (&col)[CPL],
                                             const bool (&genuine)[CPL], uint64_t wbase, uint32_t wi, uint32_t wleft, MomentAcc (&acc)[CPL], uint32_t cnt,
                                             int lane_d, F mask_at)
{
    auto flush_cols = [&](uint64_t w) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) moments_flush(a, w * (uint64_t)D + (uint64_t)col[k], acc[k]);
    };
    window_tail_rows(a, remaining / D, row0, a.rows.mask != nullptr, mask_at, wbase, wi, wleft, cnt, lane_d, flush_cols, [&](uint32_t r) {
        const uint32_t xr = tail_elem<W>(t, r * D + a.mom.ref);
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) moments_value(acc[k], tail_elem<W>(t, r * D + (uint32_t)col[k]), xr, 1u);
    });
}

// ---- group-by rows.  The bin of a row is the histogram's test on the key column's value (hist_bin); the key column's rows reach every
// lane of the group as the moments' reference column does (moments_ref_rows / moments_ref_value).  The entries are a table in the
// workgroup's LDS (non-returning ds_add_u32: nbins * D sums, bin-major, then nbins counts; BinTable::tab) or, for a workgroup whose
// chunks lie in more than one table, the caller's 64-bit entries themselves (gsum / gcount: the table of the chunk being decoded).
#ifndef SPRINTZ_GBY_MERGE
// what a block's 8 rows cost in atomics, both forms measured in profiles/groupby_rows.txt -- 1 (kept): where all 8 rows are valid and
// share a bin, a column does one add of the block's sum and the count lane one add of 8, an add a row otherwise; 0: an add a row
#define SPRINTZ_GBY_MERGE 1
#endif
struct GroupByCtx {
    BinTable bin;               // hist_bin's view of the key column
    HistCol key;                // lo = key_lo
    uint64_t* gsum;             // null: the sums are not selected
    uint64_t* gcount;           // null: the counts are not selected
    uint32_t D;
};
__device__ __forceinline__ void groupby_of_chunk(const DecodeArgs& a, GroupByCtx& c, uint64_t chunk)
{
    const uint64_t t = table_of_chunk(a, chunk);
    c.gsum = a.gby.sum ? a.gby.sum + t * ((uint64_t)a.table.nbins * (uint32_t)a.D) : nullptr;
    c.gcount = a.gby.count ? a.gby.count + t * (uint64_t)a.table.nbins : nullptr;
}
// v: one row's value, a block's sum (8 rows: below 2^19) or a run's value times its rows
__device__ __forceinline__ void groupby_add_sum(const GroupByCtx& c, uint32_t b, uint32_t col, uint64_t v) { table_add(c.bin, b * c.D + col, c.gsum, b * c.D + col, v); }
__device__ __forceinline__ void groupby_add_count(const GroupByCtx& c, uint32_t b, uint32_t n) { table_add(c.bin, c.bin.nbins * c.D + b, c.gcount, b, n); }
// a block's 8 rows: at(k, i) is this lane's row i of slot k (garbage above bit W allowed), xk the key column's rows (clean: every lane of
// the group has them from moments_ref_rows), bit i of m: row i is selected.  One lane of the group adds the counts
template <int W, int CPL, typename F>
__device__ __forceinline__ void groupby_rows8(const GroupByCtx& c, F at, const uint32_t (&xk)[8], uint32_t m, const int (&col)[CPL],
                                              const bool (&genuine)[CPL], int lane_d)
{
    uint32_t b[8], diff = 0, valid = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        b[i] = hist_bin<W>(c.bin, c.key, xk[i]);
        diff |= b[i] ^ b[0];
        valid |= (b[i] < c.bin.nbins ? 1u : 0u) << i;
    }
    valid &= m;
    if (valid == 0) return;
    if (SPRINTZ_GBY_MERGE == 1 && valid == 0xffu && diff == 0) {
        if (c.gsum) {
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (!genuine[k]) continue;
                uint32_t bs = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) bs += at(k, i) & Elem<W>::MASK;
                groupby_add_sum(c, b[0], (uint32_t)col[k], bs);
            }
        }
        if (c.gcount && lane_d == 0) groupby_add_count(c, b[0], 8u);
        return;
    }
    if (c.gsum) {
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
#pragma unroll
            for (int i = 0; i < 8; i++)
                if ((valid >> i) & 1u) groupby_add_sum(c, b[i], (uint32_t)col[k], at(k, i) & Elem<W>::MASK);
        }
    }
    if (c.gcount && lane_d == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if ((valid >> i) & 1u) groupby_add_count(c, b[i], 1u);
    }
}
// one row that `n` selected rows repeat (a delta run's constant row): xk is the key column's value, pv the lane's slots
template <int W, int CPL>
__device__ __forceinline__ void groupby_value(const GroupByCtx& c, const uint32_t (&pv)[CPL], uint32_t xk, uint32_t n, const int (&col)[CPL],
                                              const bool (&genuine)[CPL], int lane_d)
{
    const uint32_t b = hist_bin<W>(c.bin, c.key, xk);
    if (b >= c.bin.nbins || n == 0) return;
    if (c.gsum) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) groupby_add_sum(c, b, (uint32_t)col[k], (uint64_t)(pv[k] & Elem<W>::MASK) * n);
    }
    if (c.gcount && lane_d == 0) groupby_add_count(c, b, n);
}
// the workgroup's table holds its nbins * D sums, then its nbins counts (table_begin .. table_end)
__device__ __forceinline__ GroupByCtx groupby_begin(const DecodeArgs& a, uint8_t* smem)
{
    return GroupByCtx{table_begin(a, smem), HistCol{a.gby.key_lo, 0u}, a.gby.sum, a.gby.count, (uint32_t)a.D};
}
__device__ __forceinline__ void groupby_end(const DecodeArgs& a, const GroupByCtx& c)
{
    GroupByCtx g = c;
    groupby_of_chunk(a, g, (uint64_t)blockIdx.x * a.table.wg_chunks);
    table_end(a, c.bin, g.gsum, a.table.nbins * (uint32_t)a.D, g.gcount);
}
// The verbatim tail (masked_tail_rows).  The key column's element is read from the tail itself: no lane needs another's.
template <int W, int CPL, typename F>
__device__ __forceinline__ void groupby_tail(const DecodeArgs& a, const GroupByCtx& c, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0,
                                             const int (&col)[CPL], const bool (&genuine)[CPL], int lane_d, F mask_at)
{
    masked_tail_rows(remaining / D, row0, a.rows.mask != nullptr, mask_at, [&](uint32_t r, bool on) {
        if (!on) return;
        const uint32_t b = hist_bin<W>(c.bin, c.key, tail_elem<W>(t, r * D + a.gby.key));
        if (b >= c.bin.nbins) return;
        if (c.gsum) {
#pragma unroll
            for (int k = 0; k < CPL; k++)
                if (genuine[k]) groupby_add_sum(c, b, (uint32_t)col[k], tail_elem<W>(t, r * D + (uint32_t)col[k]));
        }
        if (c.gcount && lane_d == 0) groupby_add_count(c, b, 1u);
    });
}

// ---- extrema rows.  A column keeps the window's minimum and maximum with the chunk-relative rows of their first occurrences, and its
// values in the window's first and last selected rows.  The running minimum starts above every element (all ones in 32 bits) and the
// running maximum below every element (-1), so that the first selected row always takes both positions -- a selected 0xFFFF is a
// minimum with a row, a selected 0 a maximum with a row; the flush turns them into the identities the outputs hold (min all ones of
// the element type, max 0).  Value and position stay apart: no window is too long for them.
#ifndef SPRINTZ_EXT_RUN_SHORTCUT
// 1 (kept): decode_fast.h crosses a delta run in O(windows) (run_selected_span); 0: it replays the run block by block, as FIRE runs are
// -- both measured in profiles/extrema_rows.txt
#define SPRINTZ_EXT_RUN_SHORTCUT 1
#endif
struct ExtremaAcc {
    uint32_t mn, amin;
    int32_t mx;
    uint32_t amax;
    uint32_t first, last;
};
// the window's first and last selected rows (chunk-relative): the same in every lane of the group
struct ExtremaRows { uint32_t first, last; };
__device__ __forceinline__ ExtremaAcc extrema_identity() { return ExtremaAcc{0xffffffffu, kExtNoRow, -1, kExtNoRow, 0u, 0u}; }
// A column's 8 rows of one block that starts at chunk row `row0`; bit i of m != 0: row i is selected; x(i) may carry garbage above bit
// W.  Inside the block value and row share one 32-bit key under an unsigned minimum -- (x << (32 - W)) | i for the minimum,
// (~x << (32 - W)) | i for the maximum: one shift-or and one v_min_u32 a sample each, and the first occurrence wins a tie -- and the
// block's winner meets the window's under a strict compare, so an earlier block keeps a tie too.  (The row inside a BLOCK needs 3 bits:
// unlike a key that holds the row inside the window, this one sets no limit on the window's length.)
// `fresh`: the window has no selected row yet (w.first == kExtNoRow); `ends`: first / last are selected (wave-uniform).
template <int W, typename F>
__device__ __forceinline__ void extrema_rows8(ExtremaAcc& acc, F x, uint32_t m, uint32_t row0, bool fresh, bool ends)
{
    constexpr int S = 32 - W;                               // the shift drops the garbage above bit W
    uint32_t kmin = 0xffffffffu, kmax = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        // a row's constant: its number, or all ones where it is not selected -- the identity of both minima (once a block, whatever the columns)
        const uint32_t c = ((m >> i) & 1u) ? (uint32_t)i : 0xffffffffu;
        const uint32_t lo = (x(i) << S) | c;
        const uint32_t hi = (~x(i) << S) | c;                // the maximum as the minimum of the complement: the first occurrence wins there too
        kmin = lo < kmin ? lo : kmin;
        kmax = hi < kmax ? hi : kmax;
    }
    const uint32_t bmin = kmin >> S, bmax = Elem<W>::MASK - (kmax >> S);
    if (bmin < acc.mn) { acc.mn = bmin; acc.amin = row0 + (kmin & 7u); }
    if ((int32_t)bmax > acc.mx) { acc.mx = (int32_t)bmax; acc.amax = row0 + (kmax & 7u); }
    if (ends) {
        // the highest set bit's row is the last one so far; the lowest set bit's row is the first one, if the window had none
#pragma unroll
        for (int i = 0; i < 8; i++)
            if ((m >> i) & 1u) acc.last = x(i) & Elem<W>::MASK;
        if (fresh) {
#pragma unroll
            for (int i = 7; i >= 0; i--)
                if ((m >> i) & 1u) acc.first = x(i) & Elem<W>::MASK;
        }
    }
}
// the window's first / last selected rows after a block of 8 rows at row0 whose mask byte is m != 0
__device__ __forceinline__ void extrema_rows8_done(ExtremaRows& w, uint32_t m, uint32_t row0)
{
    if (w.first == kExtNoRow) w.first = row0 + (uint32_t)__ffs((int)m) - 1u;
    w.last = row0 + 31u - (uint32_t)__clz((int)m);
}
// one value x (clean) that selected rows hold of which the first is row `f` and the last row `l` (a delta run's constant row in one
// window; a row of the tail: f == l); `fresh` as above
__device__ __forceinline__ void extrema_value(ExtremaAcc& acc, uint32_t x, uint32_t f, bool fresh)
{
    if (x < acc.mn) { acc.mn = x; acc.amin = f; }
    if ((int32_t)x > acc.mx) { acc.mx = (int32_t)x; acc.amax = f; }
    if (fresh) acc.first = x;
    acc.last = x;
}
__device__ __forceinline__ void extrema_value_done(ExtremaRows& w, uint32_t f, uint32_t l)
{
    if (w.first == kExtNoRow) w.first = f;
    w.last = l;
}
// The selected rows among the 8 * nblocks that a delta run repeats from block first_block of the chunk on (run_selected_rows), and the
// chunk-relative rows of the first and the last of them (valid where the count is not 0): a group-wide find-first-set / find-last-set
// over those mask bytes -- or the run's first and last rows where mask_bytes is null.  EVERY lane of the group must come here.
__device__ __forceinline__ uint32_t run_selected_span(const uint8_t* mask_bytes, uint32_t first_block, uint32_t nblocks, int lane_d, int DP, uint32_t& f, uint32_t& l)
{
    if (!mask_bytes) {
        f = 8u * first_block;
        l = 8u * (first_block + nblocks) - 1u;
        return 8u * nblocks;
    }
    uint32_t c = 0, lo = kExtNoRow, hi = 0;
    for (uint32_t j = (uint32_t)lane_d; j < nblocks; j += (uint32_t)DP) {
        const uint32_t m = (uint32_t)mask_bytes[first_block + j];
        if (m == 0) continue;
        c += (uint32_t)__popc(m);
        const uint32_t r0 = 8u * (first_block + j);
        const uint32_t a = r0 + (uint32_t)__ffs((int)m) - 1u, b = r0 + 31u - (uint32_t)__clz((int)m);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    for (int off = DP >> 1; off > 0; off >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)lo, off, DP), b = (uint32_t)__shfl_xor((int)hi, off, DP);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    f = lo;
    l = hi;
    return group_sum(c, DP);
}
// one column's entries of one window leave (each entry has exactly one writer -- no atomics), and the accumulators start over
template <int W>
__device__ __forceinline__ void extrema_flush(const DecodeArgs& a, uint64_t idx, ExtremaAcc& acc)
{
    using U = typename Elem<W>::U;
    if (a.win.min) ((U*)a.win.min)[idx] = (U)acc.mn;
    if (a.win.max) ((U*)a.win.max)[idx] = (U)(acc.mx < 0 ? 0 : acc.mx);
    if (a.ext.argmin) a.ext.argmin[idx] = acc.amin;
    if (a.ext.argmax) a.ext.argmax[idx] = acc.amax;
    if (a.ext.first) ((U*)a.ext.first)[idx] = (U)acc.first;
    if (a.ext.last) ((U*)a.ext.last)[idx] = (U)acc.last;
    acc = extrema_identity();
}
// the window's two rows leave with its other entries (one lane of the group), and start over
__device__ __forceinline__ void extrema_rows_flush(const DecodeArgs& a, uint64_t widx, ExtremaRows& w, int lane_d)
{
    if (a.ext.rows && lane_d == 0) {
        a.ext.rows[2 * widx] = w.first;
        a.ext.rows[2 * widx + 1] = w.last;
    }
    w = ExtremaRows{kExtNoRow, kExtNoRow};
}
// The verbatim tail (window_tail_rows): a selected row's elements reach the lane's genuine columns, its number the window's rows
template <int W, int CPL, typename F>
__device__ __forceinline__ void extrema_tail(const DecodeArgs& a, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0, const int (&col)[CPL],
                                             const bool (&genuine)[CPL], uint64_t wbase, uint32_t wi, uint32_t wleft, ExtremaAcc (&acc)[CPL], ExtremaRows& wr,
                                             uint32_t cnt, int lane_d, F mask_at)
{
    auto flush_cols = [&](uint64_t w) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) extrema_flush<W>(a, w * (uint64_t)D + (uint64_t)col[k], acc[k]);
        extrema_rows_flush(a, w, wr, lane_d);
    };
    window_tail_rows(a, remaining / D, row0, a.rows.mask != nullptr, mask_at, wbase, wi, wleft, cnt, lane_d, flush_cols, [&](uint32_t r) {
        const bool fresh = wr.first == kExtNoRow;
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) extrema_value(acc[k], tail_elem<W>(t, r * D + (uint32_t)col[k]), row0 + r, fresh);
        extrema_value_done(wr, row0 + r, row0 + r);
    });
}

// ---- segment rows (Q == kQuerySegment; sprintz_mi355x_segment_rows): the aggregate mode with windows whose edges come from the mask.  Its
// arguments share structs that are here: the mask is RowMaskArgs'; min / max / sum, the per-segment row count (win.row_count) and the
// selected ops are WindowArgs', whose `rows` carries the segmentation rule (this mode has no W) and whose `count` is unused; the places
// are SelectArgs' -- segment i of chunk c at bases[c] + i, dropped at or above capacity, its first batch row c * rpc + s_i in ids.
// The rule (kSegRuns: the maximal runs of set bits; kSegSplits: every row belongs to a segment and a set bit opens a new one) decides
// per row whether it is a member and whether it starts a segment; a segment ends in front of the first row behind its start that is
// not a member or is a start, or with the chunk's rows.  What a lane group knows of its chunk's walk (the same in every lane):
constexpr uint32_t kSegRuns = 0, kSegSplits = 1;
#ifndef SPRINTZ_SEG_RUN_SHORTCUT
// 1 (kept): decode_fast.h crosses a delta run whose mask bytes hold no start and no end in O(1) (segment_run_plain); 0: it replays every
// run block by block, as FIRE runs are -- both measured in profiles/segment_rows.txt
#define SPRINTZ_SEG_RUN_SHORTCUT 1
#endif
struct SegState {
    uint32_t open;              // a segment is open: it started at chunk row `start`, and has had no end yet
    uint32_t start;
    uint32_t rank;              // the segments of the chunk that have ended = the open one's number
};
// 8 rows under mask byte m behind state `open`: bit i of members -- row i belongs to a segment; of starts -- it starts one; of ends -- the
// segment open in front of row i ends there
struct SegBlock { uint32_t members, starts, ends; };
__device__ __forceinline__ SegBlock segment_block(uint32_t mode, uint32_t m, uint32_t open)
{
    if (mode == kSegSplits) return SegBlock{0xffu, m | (open ? 0u : 1u), m & (open ? 0xffu : 0xfeu)};
    const uint32_t prev = ((m << 1) | (open ? 1u : 0u)) & 0xffu;                // bit i: row i - 1 is a member
    return SegBlock{m, m & ~prev, ~m & prev};
}
// a block with no start and no end, of members alone or of none: the accumulators take all 8 rows, or nothing happens at all
__device__ __forceinline__ bool segment_block_plain(const SegBlock& b) { return (b.starts | b.ends) == 0 && (b.members == 0xffu || b.members == 0); }
// one column's entries of the segment at `place` leave (each entry has one writer -- no atomics), and the accumulators start over from the
// identities: what they hold while no segment is open
template <int W>
__device__ __forceinline__ void segment_flush(const DecodeArgs& a, uint64_t place, uint32_t D, uint32_t col, uint32_t& qmin, uint32_t& qmax, uint64_t& qsum)
{
    using U = typename Elem<W>::U;
    if (place < a.select.capacity) {
        const uint64_t idx = place * (uint64_t)D + col;
        if (a.win.ops & 1u) ((U*)a.win.min)[idx] = (U)qmin;
        if (a.win.ops & 2u) ((U*)a.win.max)[idx] = (U)qmax;
        if (a.win.ops & 4u) a.win.sum[idx] = qsum;
    }
    qmin = Elem<W>::MASK;
    qmax = 0;
    qsum = 0;
}
// the segment's length and its first batch row leave with its other entries (one lane of the group: one writer an entry)
__device__ __forceinline__ void segment_flush_rows(const DecodeArgs& a, uint64_t place, uint64_t start, uint32_t rows, int lane_d)
{
    if (lane_d != 0 || place >= a.select.capacity) return;
    if (a.win.row_count) a.win.row_count[place] = rows;
    if (a.select.ids) a.select.ids[place] = start;
}
// one column's 8 rows x(i) (garbage above bit W allowed) of the block `b`, behind the columns of the group's state `st` (which
// segment_block_done moves on once, behind all columns): every end inside the block is a flush of the column's entries, at the places
// base + st.rank, + 1, ...; the rows between belong to the accumulators where they are members (aggregate_row)
template <int W, typename F>
__device__ __forceinline__ void segment_rows8(const DecodeArgs& a, const SegBlock& b, const SegState& st, uint64_t base, uint32_t D, uint32_t col, bool genuine,
                                              F x, uint32_t& qmin, uint32_t& qmax, uint64_t& qsum)
{
    using U = typename Elem<W>::U;
    uint32_t bs = 0;
    const uint64_t place = base + st.rank;
    // the places the block's ends may still take below capacity, and the first one's entry: an end moves on by one place and D entries
    uint32_t room = place < a.select.capacity ? (uint32_t)(a.select.capacity - place < 8u ? a.select.capacity - place : 8u) : 0u;
    if (!genuine) room = 0;
    uint64_t idx = place * (uint64_t)D + col;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if ((b.ends >> i) & 1u) {
            qsum += bs;
            bs = 0;
            if (room != 0) {
                if (a.win.ops & 1u) ((U*)a.win.min)[idx] = (U)qmin;
                if (a.win.ops & 2u) ((U*)a.win.max)[idx] = (U)qmax;
                if (a.win.ops & 4u) a.win.sum[idx] = qsum;
                room--;
            }
            idx += D;
            qmin = Elem<W>::MASK;
            qmax = 0;
            qsum = 0;
        }
        aggregate_row<W>(x(i), aggregate_sel<W>(b.members, i), qmin, qmax, bs);
    }
    qsum += bs;
}
// behind a block's columns: the ended segments' lengths and starts leave, and the state moves over the 8 rows from chunk row row0 on
// (srow0: the batch row of the chunk's row 0)
__device__ __forceinline__ void segment_block_done(const DecodeArgs& a, const SegBlock& b, SegState& st, uint64_t base, uint64_t srow0, uint32_t row0, int lane_d)
{
    if ((b.starts | b.ends) == 0) return;
    for (uint32_t i = 0; i < 8u; i++) {
        if ((b.ends >> i) & 1u) {
            segment_flush_rows(a, base + st.rank, srow0 + st.start, row0 + i - st.start, lane_d);
            st.rank++;
            st.open = 0;
        }
        if ((b.starts >> i) & 1u) {
            st.start = row0 + i;
            st.open = 1;
        }
    }
}
// Do the 8 * nblocks rows that a delta run repeats from block first_block of the chunk on hold no start and no end -- all of them members
// of the open segment, or none a member of any?  One strided pass over those mask bytes, spread over the group's lanes.  EVERY lane of
// the group must come here: the answer is a group reduction.
__device__ __forceinline__ bool segment_run_plain(uint32_t mode, const uint8_t* mask_bytes, uint32_t first_block, uint32_t nblocks, uint32_t open, int lane_d, int DP)
{
    if (mode == kSegSplits && !open) return false;             // the chunk's row 0 starts a segment
    const uint32_t want = (mode == kSegRuns && open) ? 0xffu : 0u;
    uint32_t diff = 0;
    for (uint32_t j = (uint32_t)lane_d; j < nblocks; j += (uint32_t)DP) diff |= (uint32_t)mask_bytes[first_block + j] ^ want;
    for (int off = DP >> 1; off > 0; off >>= 1) diff |= (uint32_t)__shfl_xor((int)diff, off, DP);
    return diff == 0;
}
// The verbatim tail (masked_tail_rows) and the chunk's end: every whole row of the tail walks the rule -- an end flushes, a start opens, a
// member's elements reach the accumulators of the lane's genuine columns -- and then the segment still open ends with the chunk's rows.
template <int W, int CPL, typename F>
__device__ __forceinline__ void segment_tail(const DecodeArgs& a, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0, const int (&col)[CPL],
                                             const bool (&genuine)[CPL], SegState st, uint64_t base, uint64_t srow0, uint32_t (&qmin)[CPL], uint32_t (&qmax)[CPL],
                                             uint64_t (&qsum)[CPL], int lane_d, F mask_at)
{
    const uint32_t mode = a.win.rows, nfull = remaining / D;
    auto close = [&](uint32_t end) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (genuine[k]) segment_flush<W>(a, base + st.rank, D, (uint32_t)col[k], qmin[k], qmax[k], qsum[k]);
        segment_flush_rows(a, base + st.rank, srow0 + st.start, end - st.start, lane_d);
        st.rank++;
        st.open = 0;
    };
    masked_tail_rows(nfull, row0, true, mask_at, [&](uint32_t r, bool on) {
        const bool member = mode == kSegSplits || on;
        const bool start = mode == kSegSplits ? (on || !st.open) : (on && !st.open);
        if (st.open && (start || !member)) close(row0 + r);
        if (start) {
            st.start = row0 + r;
            st.open = 1;
        }
        if (!member) return;
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
            const uint32_t x = tail_elem<W>(t, r * D + (uint32_t)col[k]);
            qmin[k] = x < qmin[k] ? x : qmin[k];
            qmax[k] = x > qmax[k] ? x : qmax[k];
            qsum[k] += x;
        }
    });
    if (st.open) close(row0 + nfull);
}

// ---- select rows: the places of the rows of one 8-row block (or of 8 rows of the tail) whose bits are set in m, behind `first` -- the
// chunk's base plus the set bits in front of the block
__device__ __forceinline__ uint64_t select_place(uint64_t first, uint32_t m, uint32_t row) { return first + (uint32_t)__popc(m & ((1u << row) - 1u)); }
// the row numbers of those rows: lanes 0 .. 7 of the group take a row each (groups of fewer lanes take turns); one writer an entry
__device__ __forceinline__ void select_ids(const DecodeArgs& a, uint64_t first, uint32_t m, uint64_t row0, int lane_d, int DP)
{
    if (!a.select.ids) return;
    for (uint32_t j = (uint32_t)lane_d; j < 8u; j += (uint32_t)DP) {
        const uint64_t p = select_place(first, m, j);
        if (((m >> j) & 1u) && p < a.select.capacity) a.select.ids[p] = row0 + j;
    }
}
// The verbatim tail: `remaining` elements at t, row-major from chunk row `row0` (a multiple of 8: the rows of the blocks in front).
// A partial last row is not a row.  Every selected row is copied by the group's lanes, an element each; `rank` is the number of
// the chunk's set bits in front of row0.  mask_at(b) is the chunk's mask byte b, read only where 8 b is below row0 + the tail's whole rows.
template <int W, typename F>
__device__ __forceinline__ void select_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t row0,
                                            uint64_t base, uint32_t rank, int lane_d, int DP, F mask_at)
{
    using U = typename Elem<W>::U;
    const uint32_t nfull = remaining / D;
    for (uint32_t r0 = 0; r0 < nfull; r0 += 8u) {
        const uint32_t n = nfull - r0 < 8u ? nfull - r0 : 8u;
        const uint32_t m = mask_at((row0 + r0) >> 3) & ((1u << n) - 1u);
        const uint64_t first = base + rank;
        for (uint32_t j = 0; j < n; j++) {
            if (!((m >> j) & 1u)) continue;
            const uint64_t p = select_place(first, m, j);
            if (p >= a.select.capacity) continue;
            U* const d = (U*)a.out + p * (uint64_t)D;
            for (uint32_t e = (uint32_t)lane_d; e < D; e += (uint32_t)DP) d[e] = (U)tail_elem<W>(t, (r0 + j) * D + e);
        }
        select_ids(a, first, m, chunk * (uint64_t)a.select.rpc + row0 + r0, lane_d, DP);
        rank += (uint32_t)__popc(m);
    }
}

// ---- filter rows.  A column's test is one subtract and one compare: ((x - lo) & MASK) < span with span = hi - lo + 1, or 0 where
// lo > hi ("never").  The kernels combine in the INVERTED domain of ALL -- a column contributes hit ^ inv, inv = all ones for ALL and
// 0 for ANY -- so that both modes are one OR across columns and lanes with the identity 0 (what a lane column past the last one
// contributes), and the result is un-inverted once per block.
struct FilterCol { uint32_t lo, span; };
template <int W>
__device__ __forceinline__ FilterCol filter_col(const DecodeArgs& a, int col, bool genuine)
{
    using U = typename Elem<W>::U;
    FilterCol f{0u, 0u};
    if (genuine) {
        const uint32_t lo = ((const U*)a.filter.lo)[col], hi = ((const U*)a.filter.hi)[col];
        f.lo = lo;
        f.span = lo <= hi ? hi - lo + 1u : 0u;
    }
    return f;
}
// (x may carry garbage above bit W: only its low W bits reach the masked difference)
template <int W> __device__ __forceinline__ uint32_t filter_hit(const FilterCol& f, uint32_t x) { return ((x - f.lo) & Elem<W>::MASK) < f.span ? 1u : 0u; }
__device__ __forceinline__ uint32_t filter_inv(const DecodeArgs& a) { return a.filter.mode == 0u ? 0xffffffffu : 0u; }
__device__ __forceinline__ uint32_t group_or_any(uint32_t v, int DP)
{
    for (int off = DP >> 1; off > 0; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, DP);
    return v;
}
// The verbatim tail: `remaining` elements at t, row-major from the row behind the chunk's `blocks_done` blocks.  A partial last row
// is not a row.  32 rows a trip: a lane folds its columns into one word, the group ORs the words, lanes 0 .. 3 store the trip's
// bytes; then the mask bytes of the slot's rows past the data are zeroed, spread over the lanes.  Every byte has one writer, and all
// of them lie in the chunk's mask_stride bytes: blocks_done * 8 + remaining / D rows are at most chunk_len / D (the callers check the
// tail against the slot before they come here).
template <int W, int CPL>
__device__ __forceinline__ void filter_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t blocks_done,
                                            int lane_d, int DP, const FilterCol (&fc)[CPL], const int (&col)[CPL], const bool (&genuine)[CPL], uint32_t& count)
{
    const uint32_t nfull = remaining / D, tbytes = (nfull + 7u) >> 3;
    const uint32_t inv = filter_inv(a);
    uint8_t* const mb = a.filter.mask ? a.filter.mask + chunk * (uint64_t)a.filter.mask_stride : nullptr;
    for (uint32_t r0 = 0; r0 < nfull; r0 += 32u) {
        const uint32_t n = nfull - r0 < 32u ? nfull - r0 : 32u;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
            for (uint32_t j = 0; j < n; j++) v |= (filter_hit<W>(fc[k], tail_elem<W>(t, (r0 + j) * D + (uint32_t)col[k])) ^ (inv & 1u)) << j;
        }
        v = (group_or_any(v, DP) ^ inv) & (n == 32u ? 0xffffffffu : (1u << n) - 1u);
        count += (uint32_t)__popc(v);
        if (mb) {
            for (uint32_t b = (uint32_t)lane_d; b < 4u; b += (uint32_t)DP)
                if ((r0 >> 3) + b < tbytes) mb[blocks_done + (r0 >> 3) + b] = (uint8_t)(v >> (8u * b));
        }
    }
    if (mb) {
        for (uint32_t j = blocks_done + tbytes + (uint32_t)lane_d; j < a.filter.mask_stride; j += (uint32_t)DP) mb[j] = 0;
    }
}

// ---- linear filter rows.  All arithmetic is on uint32_t: the sum wraps as two's complement does, and lo <= s <= hi, signed, is
// (s - lo) <= (hi - lo), unsigned, wherever lo <= hi.  A lane keeps the partial sums of the block's 8 rows over its own columns; the
// group adds them up once a block.  The lag term u x[g - 1] of a sample belongs to the NEXT row's sum: rows 0 .. 6 of a block hand it on
// inside the block, row 7's waits in one register a lane (`carry`) for the next block's row 0.  A chunk's first row is its own predecessor.
#ifndef SPRINTZ_LIN_RUN_SHORTCUT
// 1 (kept): a delta run is one evaluation and len bytes of 0x00 / 0xFF in decode_fast.h; 0: it is replayed block by block
// (profiles/filter_linear.txt)
#define SPRINTZ_LIN_RUN_SHORTCUT 1
#endif
struct LinearCol { uint32_t w, u; };      // a lane column past the last one: 0, 0 -- it contributes nothing, and no weight is loaded for it
struct LinearCtx {
    uint32_t base, span;        // bias - lo, hi - lo
    uint32_t never, lag;        // lo > hi; a lag term is given (words, not bools: hipcc kept bools of this mode in scratch)
};
__device__ __forceinline__ LinearCol linear_col(const DecodeArgs& a, int col, bool genuine)
{
    LinearCol c{0u, 0u};
    if (genuine) {
        c.w = (uint32_t)a.lin.w[col];
        if (a.lin.lag) c.u = (uint32_t)a.lin.lag[col];
    }
    return c;
}
__device__ __forceinline__ LinearCtx linear_ctx(const DecodeArgs& a)
{
    return LinearCtx{(uint32_t)a.lin.bias - (uint32_t)a.lin.lo, (uint32_t)a.lin.hi - (uint32_t)a.lin.lo, a.lin.lo > a.lin.hi ? 1u : 0u, a.lin.lag != nullptr ? 1u : 0u};
}
// sum: the row's sum without the bias
__device__ __forceinline__ uint32_t linear_hit(const LinearCtx& c, uint32_t sum) { return (!c.never && sum + c.base <= c.span) ? 1u : 0u; }
// what chunk `chunk` leaves for the seam pass (geom.h: linear_tmp_stride): the library's own layout
template <int W> struct LinearSlot {
    uint32_t* has;
    typename Elem<W>::U* first;
    typename Elem<W>::U* last;
};
template <int W> __device__ __forceinline__ LinearSlot<W> linear_slot(const DecodeArgs& a, uint64_t chunk, uint32_t D)
{
    using U = typename Elem<W>::U;
    uint8_t* const p = (uint8_t*)a.lin.tmp + chunk * linear_tmp_stride(W / 8, (int)D);
    return LinearSlot<W>{(uint32_t*)p, (U*)(p + 8), (U*)(p + 8) + D};
}
// a column's 8 rows of one block, x(i) (garbage above bit W allowed).  first: the block is the chunk's first -- `self` collects what row 0,
// as its own predecessor, hands to itself; next: what row 7 hands to the next block's row 0
template <int W, typename F>
__device__ __forceinline__ void linear_rows8(const LinearCol& c, F x, uint32_t lag, uint32_t first, uint32_t (&acc)[8], uint32_t& self, uint32_t& next)
{
    uint32_t xs[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        xs[i] = x(i) & Elem<W>::MASK;
        acc[i] += c.w * xs[i];
    }
    if (lag) {
        if (first) self += c.u * xs[0];
#pragma unroll
        for (int i = 0; i < 7; i++) acc[i + 1] += c.u * xs[i];
        next += c.u * xs[7];
    }
}
// behind a block's columns, every lane of the group: gsum(v) is v summed over the group's lanes.  -> the block's mask byte; the partial
// sums start over and row 7's lag term moves into `carry`
template <typename S>
__device__ __forceinline__ uint32_t linear_block(const LinearCtx& c, uint32_t (&acc)[8], uint32_t& first, uint32_t& self, uint32_t& carry, uint32_t& next, S gsum)
{
    acc[0] += first ? self : carry;
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m |= linear_hit(c, gsum(acc[i])) << i;
        acc[i] = 0;
    }
    carry = next;
    next = 0;
    self = 0;
    first = 0;
    return m;
}
// one lane of the group says whether the chunk has a row (a damaged chunk has none the seam pass may use)
__device__ __forceinline__ void linear_mark(const DecodeArgs& a, uint64_t chunk, uint32_t D, int W, uint32_t has, int lane_d)
{
    if (a.lin.lag && lane_d == 0) *(uint32_t*)((uint8_t*)a.lin.tmp + chunk * linear_tmp_stride(W / 8, (int)D)) = has;
}
// The verbatim tail, as filter_tail: `remaining` elements at t, row-major from the row behind the chunk's `blocks_done` blocks, 32 rows a
// trip, then the mask bytes of the slot's rows past the data are zeroed.  The tail's first row takes the last decoded row as its
// predecessor -- `carry`, each lane's share -- or, in a chunk that is all tail, itself; the rows behind it take the tail's previous row.
// Then, with a lag term, the chunk's last existing row leaves for the seam pass (the tail's last whole row, or pv: the last decoded one),
// its first one too where no block held it, and whether it has a row at all.
template <int W, int CPL>
__device__ __forceinline__ void linear_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t blocks_done,
                                            int lane_d, int DP, const LinearCol (&lc)[CPL], const int (&col)[CPL], const bool (&genuine)[CPL],
                                            const LinearCtx& c, uint32_t carry, const uint32_t (&pv)[CPL], uint32_t& count)
{
    using U = typename Elem<W>::U;
    const uint32_t nfull = remaining / D, tbytes = (nfull + 7u) >> 3;
    uint8_t* const mb = a.filter.mask ? a.filter.mask + chunk * (uint64_t)a.filter.mask_stride : nullptr;
    for (uint32_t r0 = 0; r0 < nfull; r0 += 32u) {
        const uint32_t n = nfull - r0 < 32u ? nfull - r0 : 32u;
        uint32_t v = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t r = r0 + j;
            uint32_t p = (r == 0 && blocks_done != 0) ? carry : 0u;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (!genuine[k]) continue;
                const uint32_t x = tail_elem<W>(t, r * D + (uint32_t)col[k]);
                p += lc[k].w * x;
                if (c.lag && (r != 0 || blocks_done == 0)) p += lc[k].u * (r != 0 ? tail_elem<W>(t, (r - 1u) * D + (uint32_t)col[k]) : x);
            }
            v |= linear_hit(c, group_sum(p, DP)) << j;
        }
        count += (uint32_t)__popc(v);
        if (mb) {
            for (uint32_t b = (uint32_t)lane_d; b < 4u; b += (uint32_t)DP)
                if ((r0 >> 3) + b < tbytes) mb[blocks_done + (r0 >> 3) + b] = (uint8_t)(v >> (8u * b));
        }
    }
    if (mb) {
        for (uint32_t j = blocks_done + tbytes + (uint32_t)lane_d; j < a.filter.mask_stride; j += (uint32_t)DP) mb[j] = 0;
    }
    if (c.lag) {
        const LinearSlot<W> s = linear_slot<W>(a, chunk, D);
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
            if (nfull != 0) {
                if (blocks_done == 0) s.first[col[k]] = (U)tail_elem<W>(t, (uint32_t)col[k]);
                s.last[col[k]] = (U)tail_elem<W>(t, (nfull - 1u) * D + (uint32_t)col[k]);
            } else if (blocks_done != 0) {
                s.last[col[k]] = (U)(pv[k] & Elem<W>::MASK);
            }
        }
        if (lane_d == 0) *s.has = (nfull != 0 || blocks_done != 0) ? 1u : 0u;
    }
}

// ---- gather rows
constexpr int64_t kErrCorrupt = -5;
constexpr int64_t kErrNoRow = -1;             // gather: the range needs a row that does not exist (SPRINTZ_E_INVALID)

// what piece slot `slot` has to do.  All of it follows from starts[range] on the device; a slot past the range's last
// chunk has nothing to do (false).  `obase` is where row 0 of the piece's CHUNK would land in `out`, in elements: negative or past
// the range's own rows for most pieces -- the row test [lo, hi) alone decides which stores happen.
struct GatherPiece {
    uint64_t range, chunk;
    uint32_t lo, hi;            // chunk-relative rows the range needs from this chunk, lo < hi <= rpc
    int64_t obase;
    bool exists;                // chunk < nchunks; if not, the range fails without a decode
};
__device__ __forceinline__ bool gather_piece(const DecodeArgs& a, uint64_t slot, GatherPiece& p)
{
    p.range = slot / a.gather.pieces;
    if (p.range >= a.gather.nranges) return false;
    const uint64_t k = slot - p.range * a.gather.pieces, R = a.gather.rpc;
    const uint64_t g0 = a.gather.starts[p.range], c0 = g0 / R;
    p.exists = c0 < a.nchunks;                      // (checked first: c0 + k cannot wrap below)
    p.chunk = 0; p.lo = 0; p.hi = 1; p.obase = 0;
    if (!p.exists) return k == 0;                   // one slot reports the missing rows
    const uint64_t first = g0 - c0 * R, end = first + a.gather.rows;   // the range, in rows from row 0 of chunk c0
    if (k * R >= end) return false;
    p.chunk = c0 + k;
    p.exists = p.chunk < a.nchunks;
    p.lo = (uint32_t)((first > k * R ? first : k * R) - k * R);
    p.hi = (uint32_t)((end < (k + 1) * R ? end : (k + 1) * R) - k * R);
    p.obase = ((int64_t)(p.range * a.gather.rows) + (int64_t)(k * R) - (int64_t)first) * (int64_t)a.D;
    return true;
}
// a failing piece leaves its code in the range's entry (the entries start at gather.rows: gather_rets_fill; the smallest code wins)
__device__ __forceinline__ void gather_fail(const DecodeArgs& a, uint64_t range, int64_t code)
{
    if (a.rets) atomicMin((long long*)&a.rets[range], (long long)code);
}
// The verbatim tail, `remaining` elements at t behind the `out_elems` the blocks held: the piece still needs rows of it -- or rows
// the stream does not hold (the short last chunk), which outranks a tail that overruns its stream but not a stream found `corrupt`
// before.  Elements [e_lo, e_hi) of the tail are the piece's, spread over the group's lanes.
template <int W>
__device__ __forceinline__ void gather_tail(const DecodeArgs& a, const GatherPiece& gp, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D,
                                            int lane_d, int DP, bool corrupt, bool overrun)
{
    using U = typename Elem<W>::U;
    if (!corrupt && (uint64_t)gp.hi * D > (uint64_t)out_elems + remaining) {
        if (lane_d == 0) gather_fail(a, gp.range, kErrNoRow);
        return;
    }
    if (corrupt || overrun) {
        if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt);
        return;
    }
    const uint32_t e_lo = gp.lo * D > out_elems ? gp.lo * D - out_elems : 0u;
    const uint32_t e_hi = gp.hi * D - out_elems;                              // <= remaining, checked above
    U* const d = (U*)a.out + (gp.obase + (int64_t)out_elems);
    for (uint32_t e = e_lo + (uint32_t)lane_d; e < e_hi; e += (uint32_t)DP) d[e] = (U)tail_elem<W>(t, e);
}

// ---- float rows (Q == kQueryFloat; sprintz_mi355x_float_rows): a plain decode whose stores convert.  Element e of chunk c, in column
// d = e % D, leaves at out[c * chunk_len + e] as z = fl32(fl32((float)v * scale[d]) + offset[d]) -- v the unsigned element, or the
// element sign-extended from W bits -- in float32, or rounded to nearest even to float16 / bfloat16.  The arguments travel in FilterArgs,
// as the linear filter's outputs do: filter.lo is the scale (float32 [D], null: all 1), filter.hi the offset (null: all 0), filter.mode the
// format (kFloatF32 / kFloatF16 / kFloatBF16, geom.h) and kFloatSignedBit.  Both roundings are IEEE float32 operations and never one fma.
__device__ __forceinline__ float float_scale(const DecodeArgs& a, uint32_t col) { return a.filter.lo ? ((const float*)a.filter.lo)[col] : 1.0f; }
__device__ __forceinline__ float float_offset(const DecodeArgs& a, uint32_t col) { return a.filter.hi ? ((const float*)a.filter.hi)[col] : 0.0f; }
// the sign bit of the element where the mode is signed, else 0: (x ^ sb) - sb sign-extends a clean x, or leaves it
template <int W> __device__ __forceinline__ uint32_t float_sign_bit(uint32_t mode) { return (mode & kFloatSignedBit) ? 1u << (W - 1) : 0u; }
// x is clean (nothing above bit W); the int -> float conversion is exact (|v| < 2^16)
__device__ __forceinline__ float float_value(uint32_t x, uint32_t sb, float s, float o)
{
#pragma clang fp contract(off)
    const float f = (float)(int)((x ^ sb) - sb);
    const float m = f * s;
    return m + o;
}
// round to nearest even on the float32 bits; a NaN (non-finite parameters alone) becomes the quiet NaN 0x7FC0
__device__ __forceinline__ uint32_t float_to_bf16(float z)
{
    const uint32_t u = __float_as_uint(z);
    const uint32_t r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc0u : r;
}
// v_cvt_f16_f32: round to nearest even, overflow to infinity, subnormals kept
__device__ __forceinline__ uint32_t float_to_f16(float z)
{
    const _Float16 h = (_Float16)z;
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
}
// one converted element to its place, plain 64-bit addresses (the generic kernel's blocks, every kernel's tail); fmt is wave-uniform
__device__ __forceinline__ void float_put(void* out, uint32_t fmt, uint64_t idx, float z)
{
    if (fmt == kFloatF32) ((float*)out)[idx] = z;
    else ((uint16_t*)out)[idx] = (uint16_t)(fmt == kFloatF16 ? float_to_f16(z) : float_to_bf16(z));
}
// The verbatim tail: `remaining` elements at t behind the chunk's `out_elems` (a multiple of 8 * D: element e of the tail is in column
// e % D), spread over the group's lanes
template <int W>
__device__ __forceinline__ void float_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D, int lane_d, int DP)
{
    const uint32_t fmt = a.filter.mode & 3u, sb = float_sign_bit<W>(a.filter.mode);
    const uint64_t base = chunk * (uint64_t)a.chunk_len + out_elems;
    for (uint32_t e = (uint32_t)lane_d; e < remaining; e += (uint32_t)DP) {
        const uint32_t d = e % D;
        float_put(a.out, fmt, base + e, float_value(tail_elem<W>(t, e), sb, float_scale(a, d), float_offset(a, d)));
    }
}
// One 16-byte piece of decoded elements (8 of 16 bits, 16 of 8) whose columns' scales and offsets the lane holds in sc / of: converted, it
// is NE / 4 pieces of float32 or NE / 8 of a 16-bit format -- store(j, piece) takes output piece j, 16 j bytes behind the first
template <int W, typename ST>
__device__ __forceinline__ void float_piece(const uint4& t, uint32_t mode, const float (&sc)[128 / W], const float (&of)[128 / W], ST store)
{
    constexpr int NE = 128 / W;
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
    const uint32_t sb = float_sign_bit<W>(mode), fmt = mode & 3u;
    float z[NE];
#pragma unroll
    for (int j = 0; j < NE; j++) {
        const uint32_t x = W == 16 ? (w[j >> 1] >> (16 * (j & 1))) & 0xffffu : (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        z[j] = float_value(x, sb, sc[j], of[j]);
    }
    if (fmt == kFloatF32) {
#pragma unroll
        for (int q = 0; q < NE / 4; q++)
            store(q, make_uint4(__float_as_uint(z[4 * q]), __float_as_uint(z[4 * q + 1]), __float_as_uint(z[4 * q + 2]), __float_as_uint(z[4 * q + 3])));
    } else {
        uint32_t h[NE / 2];
#pragma unroll
        for (int j = 0; j < NE / 2; j++)
            h[j] = fmt == kFloatF16 ? float_to_f16(z[2 * j]) | (float_to_f16(z[2 * j + 1]) << 16) : float_to_bf16(z[2 * j]) | (float_to_bf16(z[2 * j + 1]) << 16);
#pragma unroll
        for (int q = 0; q < NE / 8; q++) store(q, make_uint4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]));
    }
}

// ---- project rows (Q == kQueryProject; sprintz_mi355x_project_rows): a plain decode, or float rows, that stores K of the D columns.  Row r
// of chunk c is row c * R + r of a dense [rows, K] output, R = chunk_len / D, and column d leaves at slot slots[d] of it -- or nowhere: any
// table entry outside 0 .. K - 1 (tested unsigned) is "not selected", so a bad table misplaces data inside the output and never writes
// outside it.  The arguments travel in FilterArgs, as float rows' do: filter.lo / filter.hi the scale and the offset of every SLOT (float32
// [K], or null), filter.mode float rows' word with kProjectRawBit for "the element type, unconverted", filter.mask the slot table (int32
// [D]) and filter.mask_stride K.
__device__ __forceinline__ uint32_t project_k(const DecodeArgs& a) { return a.filter.mask_stride; }
__device__ __forceinline__ int32_t project_slot(const DecodeArgs& a, uint32_t col) { return ((const int32_t*)a.filter.mask)[col]; }
// one element to place idx of the output, plain 64-bit addresses (the generic kernel's blocks, every kernel's tail); mode is wave-uniform
template <int W>
__device__ __forceinline__ void project_put(const DecodeArgs& a, uint64_t idx, uint32_t x, uint32_t slot)
{
    using U = typename Elem<W>::U;
    const uint32_t mode = a.filter.mode;
    if (mode & kProjectRawBit) ((U*)a.out)[idx] = (U)x;
    else float_put(a.out, mode & 3u, idx, float_value(x, float_sign_bit<W>(mode), float_scale(a, slot), float_offset(a, slot)));
}
// The verbatim tail: `remaining` elements at t behind the chunk's `out_elems` (a multiple of 8 * D: element e of the tail is in row
// out_elems / D + e / D and column e % D), spread over the group's lanes.  Only elements that exist are written: a batch that ends
// mid-row leaves the rest of that output row as it was.
template <int W>
__device__ __forceinline__ void project_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D, int lane_d, int DP)
{
    const uint32_t K = project_k(a);
    const uint64_t row0 = chunk * (uint64_t)(a.chunk_len / D) + out_elems / D;
    for (uint32_t e = (uint32_t)lane_d; e < remaining; e += (uint32_t)DP) {
        const uint32_t slot = (uint32_t)project_slot(a, e % D);
        if (slot < K) project_put<W>(a, (row0 + e / D) * (uint64_t)K + slot, tail_elem<W>(t, e), slot);
    }
}

// ---- rolling rows (Q == kQueryRolling; sprintz_mi355x_rolling_rows): element e of chunk c, in row r = e / D and column d = e % D, leaves at
// place c * chunk_len + e of every selected output as op(x[max(0, r - W + 1) .. r, d]) -- the minimum and the maximum in the element type, the
// sum as a uint32 -- in place of the element itself.  The window is clipped at the chunk's row 0 inside the launch; the seam pass
// (decode_rolling.hip) grows the first W - 1 rows of every chunk behind the first by the rows of the chunk in front.  The mode has no struct of its
// own (DecodeArgs has no spare byte): W, the ops (kRollMin | kRollMax | kRollSum) and the outputs travel in WindowArgs (rows, ops, min, max and sum
// -- read as uint32_t*), the seam scratch in LinearArgs::tmp (null: one chunk, no seam pass), the ring's place in the launch's LDS in
// BinTableArgs::table_off.
// A chunk's history ring holds its last W + 8 raw rows, column by column: column d's rows at elements [d * (W + 8), (d + 1) * (W + 8)), row r in
// slot r % (W + 8).  W + 8 is a multiple of 8, so a block of 8 rows never wraps, and when block b arrives the W rows in front of it are all
// there.  A column belongs to one lane from the chunk's first row to its last, so a lane reads only what it wrote: the ring needs no barrier.  It
// starts cold with every chunk -- no slot is read before the chunk wrote it.
template <int W> __device__ __forceinline__ typename Elem<W>::U* rolling_ring(uint8_t* ring, const DecodeArgs& a, uint32_t col)
{
    return (typename Elem<W>::U*)ring + (size_t)col * (a.win.rows + 8u);
}
// One block: the 8 new rows x(0 .. 7) of a column, block `blk` of the chunk (rows 8 blk .. 8 blk + 7), whose row 0 is element `e0` of the batch.
// The sum is S += x[r] - x[r - W], the row that leaves read from the ring.  The minimum / maximum of row j is made of three parts: the
// suffix of rows j + 1 .. 7 of the block W / 8 back, the whole blocks in between -- common to the 8 rows -- and the prefix of rows 0 .. j of the
// new block.  The blocks in between are re-read from the ring's raw rows, W - 8 ring reads a block and column: their minima are not kept (the
// ring stays (W + 8) D elements, and the lane needs no further state than S).  A block whose window reaches in front of row 0 has fewer parts.
// put(op, j, v): row j's result v of op (kRollMin / kRollMax / kRollSum, a selected one) -- the generic kernel stores it at its place, decode_fast.h
// keeps it for its staging passes
template <int W, typename F, typename P>
__device__ __forceinline__ void rolling_step8(const DecodeArgs& a, typename Elem<W>::U* rc, uint32_t blk, F x, uint32_t& S, bool settled, P put)
{
    using U = typename Elem<W>::U;
    constexpr uint32_t MASK = Elem<W>::MASK;
    const uint32_t wb = a.win.rows >> 3, nb = wb + 1u;          // blocks of a window, of the ring
    const uint32_t slot = blk % nb;
    const bool leaving = blk >= wb;                             // the block W rows back exists: it lies in the slot the NEXT block takes
    const U* const ob = rc + 8u * (slot + 1u == nb ? 0u : slot + 1u);
    uint32_t xs[8], old[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        xs[i] = x(i) & MASK;
        old[i] = settled ? xs[i] : leaving ? (uint32_t)ob[i] : 0u;      // (settled: the ring holds this one value in every slot -- see below)
    }
    if (a.win.ops & kRollSum) {
        uint32_t s = S;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            s += xs[i] - old[i];
            put(kRollSum, i, s);
        }
        S = s;
    }
    if (a.win.ops & (kRollMin | kRollMax)) {
        // the whole blocks in between: blk - wb + 1 .. blk - 1, those of them the chunk has
        uint32_t mn = MASK, mx = 0;
        const uint32_t nmid = settled ? 0u : blk < wb - 1u ? blk : wb - 1u;
        uint32_t ms = slot;
        for (uint32_t j = 0; j < nmid; j++) {
            ms = ms == 0 ? nb - 1u : ms - 1u;
            const U* const mb = rc + 8u * ms;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t y = mb[i];
                mn = y < mn ? y : mn;
                mx = y > mx ? y : mx;
            }
        }
        // the suffixes of the block that leaves: smn[j] over its rows j + 1 .. 7 (the identities where it does not exist)
        uint32_t smn[8], smx[8];
        uint32_t rn = MASK, rx = 0;
#pragma unroll
        for (int j = 7; j >= 0; j--) {
            smn[j] = rn;
            smx[j] = rx;
            if (leaving || settled) {
                rn = old[j] < rn ? old[j] : rn;
                rx = old[j] > rx ? old[j] : rx;
            }
        }
        // the prefixes of the new block run on from the blocks in between
#pragma unroll
        for (int j = 0; j < 8; j++) {
            mn = xs[j] < mn ? xs[j] : mn;
            mx = xs[j] > mx ? xs[j] : mx;
            if (a.win.ops & kRollMin) put(kRollMin, j, smn[j] < mn ? smn[j] : mn);
            if (a.win.ops & kRollMax) put(kRollMax, j, smx[j] > mx ? smx[j] : mx);
        }
    }
    if (settled) return;
    U* const nbk = rc + 8u * slot;
#pragma unroll
    for (int i = 0; i < 8; i++) nbk[i] = (U)xs[i];
}
// the generic kernel's form: every result leaves at once, at a plain 64-bit address; e0 is the batch element of the block's row 0 in this column
template <int W, typename F>
__device__ __forceinline__ void rolling_rows8(const DecodeArgs& a, typename Elem<W>::U* rc, uint32_t blk, F x, uint32_t& S, uint64_t e0, uint32_t D, bool settled = false)
{
    using U = typename Elem<W>::U;
    rolling_step8<W>(a, rc, blk, x, S, settled, [&](uint32_t op, int j, uint32_t v) {
        const uint64_t e = e0 + (uint64_t)j * D;
        if (op == kRollSum) ((uint32_t*)a.win.sum)[e] = v;
        else if (op == kRollMin) ((U*)a.win.min)[e] = (U)v;
        else ((U*)a.win.max)[e] = (U)v;
    });
}
// Delta runs.  A delta run repeats the previous row: once W + 8 consecutive rows of a run lie behind a block -- nb = W / 8 + 1 run blocks, so that
// every slot of the ring, the leaving block's included, holds the column's one value c -- the next run block is `settled`: rolling_rows8 takes
// the leaving block and the blocks in between as c without reading them and leaves the ring as it is; S stays W c.  `done` counts the run blocks
// behind a block in a row (the kernel resets it at every block that is not one of a delta run).  A first form -- a branch of its own that stored
// the constants -- cost the uint16 x 8 delta kernel 32 registers and a wave a SIMD, and was slower than no shortcut; this one shares the step's
// stores.  Timed both ways on constant data (-DSPRINTZ_ROLL_RUN_SHORTCUT=0 is the per-block path alone): profiles/rolling_rows.txt.
#ifndef SPRINTZ_ROLL_RUN_SHORTCUT
#define SPRINTZ_ROLL_RUN_SHORTCUT 1
#endif
__device__ __forceinline__ bool rolling_run_settled(const DecodeArgs& a, uint32_t done) { return done >= (a.win.rows >> 3) + 1u; }
// One row: the per-row form of the same step, for the verbatim tail -- row r of the chunk takes x; its window is read back from the ring
template <int W>
__device__ __forceinline__ void rolling_row(const DecodeArgs& a, typename Elem<W>::U* rc, uint32_t r, uint32_t x, uint32_t& S, uint64_t e)
{
    using U = typename Elem<W>::U;
    const uint32_t w = a.win.rows, cap = w + 8u;
    uint32_t slot = r % cap;
    S += x - (r >= w ? (uint32_t)rc[(r - w) % cap] : 0u);
    rc[slot] = (U)x;
    if (a.win.ops & kRollSum) ((uint32_t*)a.win.sum)[e] = S;
    if (a.win.ops & (kRollMin | kRollMax)) {
        uint32_t mn = x, mx = x;
        const uint32_t n = r + 1u < w ? r + 1u : w;
        for (uint32_t j = 1; j < n; j++) {
            slot = slot == 0 ? cap - 1u : slot - 1u;
            const uint32_t y = rc[slot];
            mn = y < mn ? y : mn;
            mx = y > mx ? y : mx;
        }
        if (a.win.ops & kRollMin) ((U*)a.win.min)[e] = (U)mn;
        if (a.win.ops & kRollMax) ((U*)a.win.max)[e] = (U)mx;
    }
}
// The verbatim tail: `remaining` elements at t behind the chunk's `out_elems` (a multiple of 8 * D: element e of the tail is in column e % D, one
// row further on than the column's previous one).  Each lane walks its own columns (`col`, a list), row by row; a partial last row has the
// columns it has, and nothing is stored for the others.
template <int W, int CPL>
__device__ __forceinline__ void rolling_tail(const DecodeArgs& a, uint64_t chunk, uint8_t* ring, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D,
                                             const int (&col)[CPL], const bool (&genuine)[CPL], uint32_t (&S)[CPL])
{
    const uint64_t base = chunk * (uint64_t)a.chunk_len + out_elems;
    const uint32_t r0 = out_elems / D;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        typename Elem<W>::U* const rc = rolling_ring<W>(ring, a, (uint32_t)col[k]);
        uint32_t r = r0;
        for (uint32_t e = (uint32_t)col[k]; e < remaining; e += D, r++) rolling_row<W>(a, rc, r, tail_elem<W>(t, e), S[k], base + e);
    }
}
// what chunk `chunk` leaves for the seam pass (geom.h: roll_tmp_stride): the library's own layout
template <int W> struct RollSlot {
    uint32_t* elems;                // the elements the chunk decoded to; 0: damaged, or empty
    typename Elem<W>::U* rows;      // [W - 1][D]: rows R - (W - 1) .. R - 1 of a full chunk (elems == chunk_len), R = chunk_len / D
};
template <int W> __device__ __forceinline__ RollSlot<W> rolling_slot(const DecodeArgs& a, uint64_t chunk)
{
    uint8_t* const p = (uint8_t*)a.lin.tmp + chunk * roll_tmp_stride(a.win.rows, a.D, W / 8);
    return RollSlot<W>{(uint32_t*)p, (typename Elem<W>::U*)(p + 16)};
}
// a chunk that is refused before its ring exists: one lane says so
template <int W> __device__ __forceinline__ void rolling_mark(const DecodeArgs& a, uint64_t chunk, int lane_d)
{
    if (a.lin.tmp && lane_d == 0) *rolling_slot<W>(a, chunk).elems = 0u;
}
// At the chunk's end, with a seam pass to come: the element count, and -- from a full chunk, the only kind that has a successor whose windows
// it can complete -- its last W - 1 rows out of the ring (W <= R: the host checks, so they exist; the ring holds the last W + 8)
template <int W, int CPL>
__device__ __forceinline__ void rolling_leave(const DecodeArgs& a, uint64_t chunk, uint8_t* ring, uint32_t elems, uint32_t D, const int (&col)[CPL],
                                              const bool (&genuine)[CPL], int lane_d)
{
    if (!a.lin.tmp) return;
    const RollSlot<W> s = rolling_slot<W>(a, chunk);
    if (lane_d == 0) *s.elems = elems;
    if (elems != a.chunk_len) return;
    const uint32_t w = a.win.rows, cap = w + 8u, first = a.chunk_len / D - (w - 1u);
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        const typename Elem<W>::U* const rc = rolling_ring<W>(ring, a, (uint32_t)col[k]);
        uint32_t slot = first % cap;
        for (uint32_t j = 0; j + 1u < w; j++) {
            s.rows[(size_t)j * D + (uint32_t)col[k]] = rc[slot];
            slot = slot + 1u == cap ? 0u : slot + 1u;
        }
    }
}

// ---- cumulative rows (Q == kQueryCumulative; sprintz_mi355x_cumulative_rows): element e of chunk c, in row r = e / D and column d = e % D, leaves at
// place c * chunk_len + e of every selected output as the column's running value from the batch's first row to its own: the minimum and the maximum
// in the element type, the sum modulo 2^64 as an int64 or its low half as an int32.  A chunk does not start from the identities but from its
// ENTERING state -- the seeds taken through every chunk in front of it -- which the scan (decode_cumulative.hip) left in a table of uint64
// [nchunks][3][D]: a min row, a max row and a sum row a chunk, the layout of the call's carries.  The mode has no struct of its own (DecodeArgs has
// no spare byte): the ops (kCumMin | kCumMax | kCumSum) and the outputs travel in WindowArgs (ops, min, max, sum), sum_bytes in WindowArgs::count,
// the table in LinearArgs::tmp (null: the identities) and -- in a call of one chunk, which has no scan: the table is then the caller's carry_in
// -- the caller's carry_out in LinearArgs::w (null: none), which the last chunk's lanes fill.
// A lane walks its column from the chunk's first row to its last, so the running values are registers: no LDS, no barrier.
struct CumState {
    uint32_t mn, mx;
    uint64_t sum;
};
template <int W> __device__ __forceinline__ CumState cumulative_enter(const DecodeArgs& a, uint64_t chunk, uint32_t D, uint32_t col)
{
    const uint64_t* const st = (const uint64_t*)a.lin.tmp;
    if (!st) return CumState{Elem<W>::MASK, 0u, 0ull};
    const uint64_t* const p = st + chunk * 3ull * D + col;
    return CumState{(uint32_t)p[0] & Elem<W>::MASK, (uint32_t)p[D] & Elem<W>::MASK, p[2u * D]};
}
__device__ __forceinline__ uint64_t* cumulative_carry_out(const DecodeArgs& a) { return (uint64_t*)const_cast<int32_t*>(a.lin.w); }
// One block: the 8 new rows x(0 .. 7) of a column.  put(op, j, v): row j's result v of op (a selected one) -- the generic kernel stores it at its
// place, decode_fast.h keeps it for its staging passes
template <int W, typename F, typename P>
__device__ __forceinline__ void cumulative_step8(const DecodeArgs& a, F x, CumState& s, P put)
{
    constexpr uint32_t MASK = Elem<W>::MASK;
    uint32_t xs[8];
#pragma unroll
    for (int i = 0; i < 8; i++) xs[i] = x(i) & MASK;
    if (a.win.ops & kCumMin) {
        uint32_t m = s.mn;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            m = xs[i] < m ? xs[i] : m;
            put(kCumMin, i, (uint64_t)m);
        }
        s.mn = m;
    }
    if (a.win.ops & kCumMax) {
        uint32_t m = s.mx;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            m = xs[i] > m ? xs[i] : m;
            put(kCumMax, i, (uint64_t)m);
        }
        s.mx = m;
    }
    if (a.win.ops & kCumSum) {
        uint64_t t = s.sum;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            t += xs[i];
            put(kCumSum, i, t);
        }
        s.sum = t;
    }
}
// one result at its place, a plain 64-bit address: batch element e
template <int W> __device__ __forceinline__ void cumulative_put(const DecodeArgs& a, uint32_t op, uint64_t e, uint64_t v)
{
    using U = typename Elem<W>::U;
    if (op == kCumMin) ((U*)a.win.min)[e] = (U)v;
    else if (op == kCumMax) ((U*)a.win.max)[e] = (U)v;
    else if (a.win.count == 8u) a.win.sum[e] = v;
    else ((uint32_t*)a.win.sum)[e] = (uint32_t)v;
}
// the generic kernel's form: every result leaves at once; e0 is the batch element of the block's row 0 in this column
template <int W, typename F>
__device__ __forceinline__ void cumulative_rows8(const DecodeArgs& a, F x, CumState& s, uint64_t e0, uint32_t D)
{
    cumulative_step8<W>(a, x, s, [&](uint32_t op, int j, uint64_t v) { cumulative_put<W>(a, op, e0 + (uint64_t)j * D, v); });
}
// The verbatim tail: `remaining` elements at t behind the chunk's `out_elems` (a multiple of 8 * D: element e of the tail is in column e % D, one
// row further on than the column's previous one).  Each lane walks its own columns (`col`, a list), row by row; a partial last row has the
// columns it has, and nothing is stored for the others.
template <int W, int CPL>
__device__ __forceinline__ void cumulative_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D,
                                                const int (&col)[CPL], const bool (&genuine)[CPL], CumState (&s)[CPL])
{
    const uint64_t base = chunk * (uint64_t)a.chunk_len + out_elems;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        for (uint32_t e = (uint32_t)col[k]; e < remaining; e += D) {
            const uint32_t x = tail_elem<W>(t, e);
            s[k].mn = x < s[k].mn ? x : s[k].mn;
            s[k].mx = x > s[k].mx ? x : s[k].mx;
            s[k].sum += x;
            if (a.win.ops & kCumMin) cumulative_put<W>(a, kCumMin, base + e, s[k].mn);
            if (a.win.ops & kCumMax) cumulative_put<W>(a, kCumMax, base + e, s[k].mx);
            if (a.win.ops & kCumSum) cumulative_put<W>(a, kCumSum, base + e, s[k].sum);
        }
    }
}
// At the chunk's end, in a call of one chunk: the state behind the chunk's last element goes to carry_out -- of a damaged chunk the state it
// entered with, since it counts as the identity.  (Only the ops asked for were kept up: the rows of the others leave as they entered.)
template <int W, int CPL>
__device__ __forceinline__ void cumulative_leave(const DecodeArgs& a, uint64_t chunk, bool damaged, uint32_t D, const int (&col)[CPL], const bool (&genuine)[CPL],
                                                 const CumState (&s)[CPL])
{
    uint64_t* const out = cumulative_carry_out(a);
    if (!out || chunk + 1 != a.nchunks) return;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        const CumState in = cumulative_enter<W>(a, chunk, D, (uint32_t)col[k]);
        const bool keep = !damaged;
        out[(uint32_t)col[k]] = keep && (a.win.ops & kCumMin) ? s[k].mn : in.mn;
        out[D + (uint32_t)col[k]] = keep && (a.win.ops & kCumMax) ? s[k].mx : in.mx;
        out[2u * D + (uint32_t)col[k]] = keep && (a.win.ops & kCumSum) ? s[k].sum : in.sum;
    }
}
// a chunk that is refused before its lanes have their columns: the group's lanes share the columns out
__device__ __forceinline__ void cumulative_mark(const DecodeArgs& a, uint64_t chunk, uint32_t D, int lane_d, int DP, int W)
{
    uint64_t* const out = cumulative_carry_out(a);
    if (!out || chunk + 1 != a.nchunks) return;
    const uint64_t mask = W == 8 ? 0xffull : 0xffffull;
    const uint64_t* const st = (const uint64_t*)a.lin.tmp;
    for (uint32_t d = (uint32_t)lane_d; d < D; d += (uint32_t)DP) {
        out[d] = st ? st[chunk * 3ull * D + d] & mask : mask;
        out[D + d] = st ? st[chunk * 3ull * D + D + d] & mask : 0ull;
        out[2u * D + d] = st ? st[chunk * 3ull * D + 2u * D + d] : 0ull;
    }
}

// ---- derive rows (Q == kQueryDerive; sprintz_mi355x_derive_rows): the linear filter's sum itself, K forms of it a row.  Row r of chunk c is row
// g = c * R + r of a dense [rows, K] output, R = chunk_len / D, and form k's value s[g, k] = bias[k] + sum_d w[k, d] x[g, d] + sum_d u[k, d] x[g - 1, d]
// (wrapping 32-bit arithmetic, the unsigned element) leaves at element g * K + k: as the int32 it is, or as fl32(fl32((float)s * scale[k]) +
// offset[k]) in float32 / float16 / bfloat16.  The arguments travel in structs that are here: LinearArgs' w and lag are the [K][D] tables and tmp the
// seam scratch (LinearSlot, as the linear filter leaves it); FilterArgs' lo / hi are the scale and the offset of every FORM (float32 [K], or null),
// mode float rows' format with kDeriveI32Bit for "the sum, unconverted", mask the biases (int32 [K], or null: all 0), counts the caller's `prev` row
// ([D], element type, or null; the seam pass alone reads it) and mask_stride K.  Inside the decode launch a chunk's first row is its own
// predecessor, as for the linear filter; with a lag term the seam pass of decode_derive.hip then writes row 0 of every chunk again.
__device__ __forceinline__ uint32_t derive_k(const DecodeArgs& a) { return a.filter.mask_stride; }
__device__ __forceinline__ uint32_t derive_bias(const DecodeArgs& a, uint32_t k) { return a.filter.mask ? (uint32_t)((const int32_t*)a.filter.mask)[k] : 0u; }
__device__ __forceinline__ const void* derive_prev(const DecodeArgs& a) { return (const void*)a.filter.counts; }
// the int32 -> float32 conversion rounds to nearest even (from |s| >= 2^24 on); both operations behind it are IEEE float32 and never one fma
__device__ __forceinline__ float derive_value(uint32_t s, float sc, float of)
{
#pragma clang fp contract(off)
    const float f = (float)(int32_t)s;
    const float m = f * sc;
    return m + of;
}
// one value to place idx of the output, plain 64-bit addresses (the generic kernel's blocks, every kernel's tail, the seam pass); mode is wave-uniform
__device__ __forceinline__ void derive_put(const DecodeArgs& a, uint64_t idx, uint32_t s, uint32_t k)
{
    const uint32_t mode = a.filter.mode;
    if (mode & kDeriveI32Bit) ((uint32_t*)a.out)[idx] = s;
    else float_put(a.out, mode & 3u, idx, derive_value(s, float_scale(a, k), float_offset(a, k)));
}
// A block's 8 rows on the generic kernel, every lane of the group: at(c, i) is row i of the lane's column slot c (clean), row0 the batch row of the
// block's row 0, `first`: the block is the chunk's first (its row 0 is its own predecessor), last[c]: the row in front of the block, and behind
// it the block's row 7.  A form at a time: the lane's partial sums of the 8 rows over its columns, the group's sums (gsum), and lane i mod DP
// stores row i's value -- no K-sized array waits in registers, whatever K is.
template <int CPL, typename F, typename S>
__device__ __forceinline__ void derive_rows8(const DecodeArgs& a, uint64_t row0, uint32_t D, int lane_d, int DP, const int (&col)[CPL], const bool (&genuine)[CPL],
                                             F at, bool first, uint32_t (&last)[CPL], S gsum)
{
    const uint32_t K = derive_k(a);
    const bool lag = a.lin.lag != nullptr;
    for (uint32_t k = 0; k < K; k++) {
        uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            if (!genuine[c]) continue;
            const uint32_t w = (uint32_t)a.lin.w[k * D + (uint32_t)col[c]];
#pragma unroll
            for (int i = 0; i < 8; i++) p[i] += w * at(c, i);
            if (lag) {
                const uint32_t u = (uint32_t)a.lin.lag[k * D + (uint32_t)col[c]];
                p[0] += u * (first ? at(c, 0) : last[c]);
#pragma unroll
                for (int i = 0; i < 7; i++) p[i + 1] += u * at(c, i);
            }
        }
        const uint32_t b = derive_bias(a, k);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t s = gsum(p[i]) + b;
            if ((uint32_t)lane_d == ((uint32_t)i & (uint32_t)(DP - 1))) derive_put(a, (row0 + (uint64_t)i) * K + k, s, k);
        }
    }
#pragma unroll
    for (int c = 0; c < CPL; c++) last[c] = at(c, 7);
}
// The verbatim tail, linear_tail's walk with values out instead of bits: `remaining` elements at t, row-major from the row behind the chunk's
// `blocks_done` blocks.  Only whole rows are rows; the tail's first row takes the last decoded row (last[c], clean) as its predecessor or, in a chunk
// that is all tail, itself; the rows behind it take the tail's previous row.  Then, with a lag term, the chunk's first and last existing rows and
// whether it has a row at all leave for the seam pass, exactly as the linear filter leaves them.
template <int W, int CPL>
__device__ __forceinline__ void derive_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t blocks_done,
                                            int lane_d, int DP, const int (&col)[CPL], const bool (&genuine)[CPL], const uint32_t (&last)[CPL])
{
    using U = typename Elem<W>::U;
    const uint32_t nfull = remaining / D, K = derive_k(a);
    const bool lag = a.lin.lag != nullptr;
    const uint64_t row0 = chunk * (uint64_t)(a.chunk_len / D) + 8ull * blocks_done;
    for (uint32_t r = 0; r < nfull; r++) {
        for (uint32_t k = 0; k < K; k++) {
            uint32_t p = 0;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                if (!genuine[c]) continue;
                const uint32_t x = tail_elem<W>(t, r * D + (uint32_t)col[c]);
                p += (uint32_t)a.lin.w[k * D + (uint32_t)col[c]] * x;
                if (lag) {
                    const uint32_t xp = r != 0 ? tail_elem<W>(t, (r - 1u) * D + (uint32_t)col[c]) : blocks_done != 0 ? last[c] : x;
                    p += (uint32_t)a.lin.lag[k * D + (uint32_t)col[c]] * xp;
                }
            }
            const uint32_t s = group_sum(p, DP) + derive_bias(a, k);
            if ((uint32_t)lane_d == (k & (uint32_t)(DP - 1))) derive_put(a, (row0 + r) * K + k, s, k);
        }
    }
    if (lag) {
        const LinearSlot<W> s = linear_slot<W>(a, chunk, D);
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            if (!genuine[c]) continue;
            if (nfull != 0) {
                if (blocks_done == 0) s.first[col[c]] = (U)tail_elem<W>(t, (uint32_t)col[c]);
                s.last[col[c]] = (U)tail_elem<W>(t, (nfull - 1u) * D + (uint32_t)col[c]);
            } else if (blocks_done != 0) {
                s.last[col[c]] = (U)last[c];
            }
        }
        if (lane_d == 0) *s.has = (nfull != 0 || blocks_done != 0) ? 1u : 0u;
    }
}

// ---- FIR rows (Q == kQueryFir; sprintz_mi355x_fir_rows): element e of chunk c, in row r = e / D and column d = e % D, leaves at place c * chunk_len + e
// of the output as y = bias[d] + sum_{j < T} taps[j][d] x[r - j, d] (wrapping 32-bit arithmetic, the unsigned element) -- as the int32 it is or converted as
// derive rows convert (derive_put, with the column's scale and offset) -- in place of the element itself.  Rows in front of the chunk's row 0 contribute
// nothing inside the launch: the seam pass (decode_fir.hip) computes the first T - 1 rows of every chunk again, wholly, from the raw rows the chunks
// leave in the scratch.  The mode has no struct of its own: T travels in WindowArgs::count and the history's rows Wh = fir_history_rows(T) in
// WindowArgs::rows -- so that the history IS rolling rows' ring (rolling_ring, roll_ring_bytes), Wh + 8 raw rows a column -- the taps ([T][D] int32) in
// LinearArgs::w, the biases ([D] int32, or null: all 0) in LinearArgs::lag, the scratch in LinearArgs::tmp (null: T == 1, no seam pass); the format, the
// scale and the offset of every COLUMN in FilterArgs' mode, lo and hi and the caller's `prev` rows in FilterArgs::counts, as derive rows carry theirs; the
// ring's place in the launch's LDS in BinTableArgs::table_off.
__device__ __forceinline__ uint32_t fir_ntaps(const DecodeArgs& a) { return a.win.count; }
__device__ __forceinline__ uint32_t fir_bias(const DecodeArgs& a, uint32_t d) { return a.lin.lag ? (uint32_t)a.lin.lag[d] : 0u; }
// what chunk `chunk` leaves for the seam pass (geom.h: fir_tmp_stride): the library's own layout
template <int W> struct FirSlot {
    uint32_t* elems;                // the elements the chunk decoded to; 0: damaged, or empty
    typename Elem<W>::U* first;     // [T - 1][D]: the chunk's rows 0 .. T - 2, those it has
    typename Elem<W>::U* last;      // [T - 1][D]: rows R - (T - 1) .. R - 1 of a full chunk (elems == chunk_len), R = chunk_len / D
};
template <int W> __device__ __forceinline__ FirSlot<W> fir_slot(const DecodeArgs& a, uint64_t chunk)
{
    using U = typename Elem<W>::U;
    uint8_t* const p = (uint8_t*)a.lin.tmp + chunk * fir_tmp_stride(fir_ntaps(a), a.D, W / 8);
    return FirSlot<W>{(uint32_t*)p, (U*)(p + 16), (U*)(p + 16) + (size_t)(fir_ntaps(a) - 1u) * (uint32_t)a.D};
}
// a ring block -- 8 rows of a column, 16 bytes (uint16) or 8 (uint8), aligned to its size -- as one LDS access, whatever type the rows were written by
template <int W> __device__ __forceinline__ void fir_block_get(const typename Elem<W>::U* b, uint32_t (&v)[8])
{
    if constexpr (W == 16) {
        uint32_t w[4];
        __builtin_memcpy(w, __builtin_assume_aligned(b, 16), 16);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    } else {
        uint32_t w[2];
        __builtin_memcpy(w, __builtin_assume_aligned(b, 8), 8);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
    }
}
template <int W> __device__ __forceinline__ void fir_block_set(typename Elem<W>::U* b, const uint32_t (&v)[8])
{
    if constexpr (W == 16) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = v[2 * i] | (v[2 * i + 1] << 16);
        __builtin_memcpy(__builtin_assume_aligned(b, 16), w, 16);
    } else {
        uint32_t w[2];
#pragma unroll
        for (int i = 0; i < 2; i++) w[i] = v[4 * i] | (v[4 * i + 1] << 8) | (v[4 * i + 2] << 16) | (v[4 * i + 3] << 24);
        __builtin_memcpy(__builtin_assume_aligned(b, 8), w, 8);
    }
}
// One block: the 8 new rows x(0 .. 7) of a column, block `blk` of the chunk (rows 8 blk .. 8 blk + 7).  They are written to the ring (and, with a seam
// pass to come, those of them among the chunk's first T - 1 rows to first[r * D]: the ring will not hold them at the chunk's end); then the 8 outputs
// are accumulated from the ring's blocks, newest to oldest.  The block m blocks back holds rows 8 (blk - m) + p; row p of it meets output i with tap
// 8 m + i - p -- the 15 taps around 8 m, those of them inside 0 .. T - 1 -- so a block is one LDS read, 15 taps and 64 multiply-adds; the new block
// itself, m = 0, takes taps 0 .. 7 and the 36 products with p <= i.  Blocks in front of the chunk's row 0 do not exist and contribute nothing.
// tap(j): the column's tap j, 0 <= j < T; put(i, y): row i's result
template <int W, typename F, typename TP, typename P>
__device__ __forceinline__ void fir_step8(const DecodeArgs& a, typename Elem<W>::U* rc, uint32_t blk, F x, TP tap, uint32_t bias, typename Elem<W>::U* first, uint32_t D, P put)
{
    using U = typename Elem<W>::U;
    constexpr uint32_t MASK = Elem<W>::MASK;
    const uint32_t T = fir_ntaps(a), nb = (a.win.rows >> 3) + 1u;      // blocks of the ring
    const uint32_t slot = blk % nb;
    uint32_t xs[8], acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) xs[i] = x(i) & MASK;
    fir_block_set<W>(rc + 8u * slot, xs);
    if (first && 8u * blk + 1u < T) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (8u * blk + (uint32_t)i + 1u < T) first[(size_t)(8u * blk + (uint32_t)i) * D] = (U)xs[i];
    }
    {
        uint32_t t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = (uint32_t)q < T ? tap((uint32_t)q) : 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t s = bias;
#pragma unroll
            for (int p = 0; p <= i; p++) s += t[i - p] * xs[p];
            acc[i] = s;
        }
    }
    const uint32_t nm = blk < nb - 1u ? blk : nb - 1u;          // the older blocks the chunk has, of those T - 1 rows reach
    uint32_t ms = slot;
    for (uint32_t m = 1; m <= nm; m++) {
        ms = ms == 0 ? nb - 1u : ms - 1u;
        uint32_t v[8], t[15];
        fir_block_get<W>(rc + 8u * ms, v);
#pragma unroll
        for (int q = 0; q < 15; q++) {
            const uint32_t j = 8u * m + (uint32_t)q - 7u;
            t[q] = j < T ? tap(j) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int p = 0; p < 8; p++) acc[i] += t[i - p + 7] * v[p];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) put(i, acc[i]);
}
// One row: the per-row form of the same step, for the verbatim tail -- row r of the chunk takes x; its history is read back from the ring
template <int W, typename TP>
__device__ __forceinline__ uint32_t fir_row(const DecodeArgs& a, typename Elem<W>::U* rc, uint32_t r, uint32_t x, TP tap, uint32_t bias, typename Elem<W>::U* first, uint32_t D)
{
    using U = typename Elem<W>::U;
    const uint32_t T = fir_ntaps(a), cap = a.win.rows + 8u;
    uint32_t slot = r % cap;
    rc[slot] = (U)x;
    if (first && r + 1u < T) first[(size_t)r * D] = (U)x;
    uint32_t y = bias + tap(0u) * x;
    const uint32_t n = r + 1u < T ? r + 1u : T;
    for (uint32_t j = 1; j < n; j++) {
        slot = slot == 0 ? cap - 1u : slot - 1u;
        y += tap(j) * (uint32_t)rc[slot];
    }
    return y;
}
// The verbatim tail: `remaining` elements at t behind the chunk's `out_elems` (a multiple of 8 * D: element e of the tail is in column e % D, one
// row further on than the column's previous one).  Each lane walks its own columns (`col`, a list), row by row, taps from global memory; a partial
// last row has the columns it has, and nothing is stored for the others.
template <int W, int CPL>
__device__ __forceinline__ void fir_tail(const DecodeArgs& a, uint64_t chunk, uint8_t* ring, const uint8_t* t, uint32_t out_elems, uint32_t remaining, uint32_t D,
                                         const int (&col)[CPL], const bool (&genuine)[CPL])
{
    using U = typename Elem<W>::U;
    const uint64_t base = chunk * (uint64_t)a.chunk_len + out_elems;
    const uint32_t r0 = out_elems / D;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        const uint32_t d = (uint32_t)col[k];
        U* const rc = rolling_ring<W>(ring, a, d);
        U* const first = a.lin.tmp ? fir_slot<W>(a, chunk).first + d : nullptr;
        const uint32_t bias = fir_bias(a, d);
        uint32_t r = r0;
        for (uint32_t e = d; e < remaining; e += D, r++)
            derive_put(a, base + e, fir_row<W>(a, rc, r, tail_elem<W>(t, e), [&](uint32_t j) { return (uint32_t)a.lin.w[(size_t)j * D + d]; }, bias, first, D), d);
    }
}
// a chunk that is refused before its ring exists: one lane says so
template <int W> __device__ __forceinline__ void fir_mark(const DecodeArgs& a, uint64_t chunk, int lane_d)
{
    if (a.lin.tmp && lane_d == 0) *fir_slot<W>(a, chunk).elems = 0u;
}
// At the chunk's end, with a seam pass to come: the element count, and -- from a full chunk, the only kind that has a successor whose first rows it
// can complete -- its last T - 1 rows out of the ring (T - 1 <= R: the host checks, so they exist; the ring holds the last Wh + 8 >= T - 1)
template <int W, int CPL>
__device__ __forceinline__ void fir_leave(const DecodeArgs& a, uint64_t chunk, uint8_t* ring, uint32_t elems, uint32_t D, const int (&col)[CPL],
                                          const bool (&genuine)[CPL], int lane_d)
{
    if (!a.lin.tmp) return;
    const FirSlot<W> s = fir_slot<W>(a, chunk);
    if (lane_d == 0) *s.elems = elems;
    if (elems != a.chunk_len) return;
    const uint32_t h = fir_ntaps(a) - 1u, cap = a.win.rows + 8u, from = a.chunk_len / D - h;
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        if (!genuine[k]) continue;
        const typename Elem<W>::U* const rc = rolling_ring<W>(ring, a, (uint32_t)col[k]);
        uint32_t slot = from % cap;
        for (uint32_t j = 0; j < h; j++) {
            s.last[(size_t)j * D + (uint32_t)col[k]] = rc[slot];
            slot = slot + 1u == cap ? 0u : slot + 1u;
        }
    }
}
// the generic kernel's form of the block step: taps from global memory, every result at once to its place, at a plain 64-bit address; e0 is the batch
// element of the block's row 0 in column d
template <int W, typename F>
__device__ __forceinline__ void fir_rows8(const DecodeArgs& a, uint64_t chunk, typename Elem<W>::U* rc, uint32_t blk, F x, uint64_t e0, uint32_t D, uint32_t d)
{
    typename Elem<W>::U* const first = a.lin.tmp ? fir_slot<W>(a, chunk).first + d : nullptr;
    fir_step8<W>(a, rc, blk, x, [&](uint32_t j) { return (uint32_t)a.lin.w[(size_t)j * D + d]; }, fir_bias(a, d), first, D,
                 [&](int i, uint32_t y) { derive_put(a, e0 + (uint64_t)i * D, y, d); });
}

}  // namespace sprintz
