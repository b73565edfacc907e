// launch.h -- host-side dispatch onto the template instantiations.  Each
// (width, direction) pair lives in its own translation unit so that hipcc can
// build them in parallel.
#pragma once

#include <hip/hip_runtime.h>

#include "lds_attr.h"
#include "decode_kernel.h"
#include "decode_fast.h"
#include "decode_uni.h"
#include "encode_kernel.h"
#include "encode_fast.h"
#include "encode_uni.h"
#include "encode_wide.h"

namespace sprintz {

// The lane-per-column decoders, one launcher a family; q is the row operation (geom.h: kQueryOff .. kQueryFir).  Each forwards to the
// translation unit that holds the instantiation -- decode_w8.hip / decode_w16.hip for the plain decode and the reduce / window
// queries, a unit of its own for every other mode (SPRINTZ_ROW_OP_UNITS below) -- so that every unit keeps its compile flags.
// generic lane mapping, both layouts, up to 512 columns (decode_kernel.h)
hipError_t launch_decode_generic(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a);
// fast path: general layout, one column per lane, LDS-transposed stores (see decode_fast.h); gather and select for rows of whole 16-byte pieces
// (ds: columns the LDS carve is sized for when that is fewer than dp * cpl -- decode_fast.h, DS; 0 = dp * cpl)
hipError_t launch_decode_fast(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a);
// low-dim streams with 1, 2 or 4 columns (8 bits) / 1 or 2 (16 bits), one lane per chunk (decode_uni.h): every mode but gather, select, aggregate, histogram, moments, group-by, extrema, the linear filter, segments, float rows, rolling rows, project rows, cumulative rows, derive rows and FIR rows
hipError_t launch_decode_uni(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a);
// internal -- the units' own entry points, reached through the three launchers above alone (api.hip).  A unit refuses a width or
// a mode it does not hold; the decode_uni units size their grid themselves (decode_uni_threads) and ignore `grid`
#define SPRINTZ_DECODE_UNIT_DECL(NAME)                                                                                                                          \
    hipError_t decode_generic_##NAME(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a);          \
    hipError_t decode_fast_##NAME(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a);
SPRINTZ_DECODE_UNIT_DECL(w8)
SPRINTZ_DECODE_UNIT_DECL(w16)
// the row operations' units, a mode each, in the order of their kQuery* numbers (api.hip builds its table of units from this list)
#define SPRINTZ_ROW_OP_UNITS(X) X(gather) X(filter) X(select) X(aggregate) X(histogram) X(moments) X(groupby) X(extrema) X(linear) X(segment) X(float) X(rolling) X(project) X(cumulative) X(derive) X(fir)
SPRINTZ_ROW_OP_UNITS(SPRINTZ_DECODE_UNIT_DECL)
hipError_t decode_uni_w8(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a);
hipError_t decode_uni_w16(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a);
hipError_t decode_uni_filter(int w, bool fire, int nd, int q, unsigned grid, hipStream_t st, const DecodeArgs& a);
// filter_row_ids: a mask of filter_rows into ascending batch row numbers, a lane group per chunk (decode_filter.hip)
hipError_t launch_filter_row_ids(const uint8_t* mask, const uint64_t* bases, uint64_t nchunks, uint32_t rows, uint64_t* ids, uint64_t capacity, hipStream_t st);
// segment_count: the segments of every chunk's mask under rule `mode`, over the rows lens (optional: element counts) says the chunk holds (decode_segment.hip)
hipError_t launch_segment_count(const uint8_t* mask, uint64_t nchunks, uint32_t rows, uint32_t D, uint32_t mode, const int64_t* lens, uint32_t* counts, hipStream_t st);
// filter_linear's seam pass: row 0 of every chunk behind the first takes the last row of the chunk in front as its predecessor (decode_linear.hip)
hipError_t launch_linear_seam(int esz, const DecodeArgs& a, hipStream_t st);
// derive_rows' seam pass: row 0 of every chunk behind the first -- and of the first, where the caller gave a `prev` row -- is computed again with its
// true predecessor and stored over what the decode left (decode_derive.hip)
hipError_t launch_derive_seam(int esz, const DecodeArgs& a, hipStream_t st);
// fir_rows' seam pass: the first T - 1 rows of every chunk are computed again, wholly, from the raw rows the chunks left in the scratch -- their own first
// rows and the last rows of the chunk in front (chunk 0: the caller's `prev` rows, or its row 0 replicated) -- and stored over what the decode left (decode_fir.hip)
hipError_t launch_fir_seam(int esz, const DecodeArgs& a, hipStream_t st);
// rolling_rows' seam pass: the first W - 1 rows of every chunk behind the first take the last rows of the chunk in front into their windows (decode_rolling.hip)
hipError_t launch_rolling_seam(int esz, const DecodeArgs& a, hipStream_t st);
// cumulative_rows' scan: the chunks' totals in d_tmp (geom.h: cum_tmp_layout) become each chunk's entering state, seeded with carry_in (null: the
// identities); a damaged chunk counts as the identity; carry_out (optional) takes the state behind the last chunk (decode_cumulative.hip)
hipError_t launch_cumulative_scan(int esz, uint64_t nchunks, uint32_t D, uint32_t ops, void* d_tmp, const uint64_t* carry_in, uint64_t* carry_out, hipStream_t st);
// small batches: one workgroup per chunk, both layouts, 1 .. 64 columns (decode_lat.h); bound_bytes = the longest stream a chunk can have
hipError_t launch_decode_lat(int w, bool fire, int dp, bool lowdim, unsigned grid, uint32_t bound_bytes, hipStream_t st, const DecodeArgs& a);
hipError_t launch_encode_lat(int w, bool fire, int dp, bool lowdim, unsigned grid, uint32_t bound_bytes, hipStream_t st, const EncodeArgs& a);   // encode_lat.h
// streams of 513 .. 2047 columns: one workgroup per chunk, <= 8 columns per lane (any_ndims.hip); shmem = the encoder's group window
hipError_t launch_decode_any(int w, bool fire, unsigned grid, hipStream_t st, const DecodeArgs& a);
hipError_t launch_encode_any(int w, bool fire, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
// streams of 2 048 .. 65 535 columns: the same scheme in column tiles, per-column state behind the rows / in `counters` (nchunks x ndims int32; FIRE only)
hipError_t launch_decode_big(int w, bool fire, unsigned grid, hipStream_t st, const DecodeArgs& a, int32_t* counters);
hipError_t launch_encode_big(int w, bool fire, unsigned grid, hipStream_t st, const EncodeArgs& a, int32_t* counters);
// streams of 65 .. 128 columns, two columns per lane (encode_wide.h)
hipError_t launch_encode_wide_w8(bool fire, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_wide_w16(bool fire, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
// two columns per lane for streams of up to 64 columns: dp = 4 / 8 / 16 / 32 lanes a chunk (encode_wide.h, DPT)
hipError_t launch_encode_pair_w8(bool fire, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_pair_w16(bool fire, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
// 8-bit streams of 65 .. 80 columns on 32 lanes a chunk (encode_wide.h, SPLIT)
hipError_t launch_encode_split_w8(bool fire, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_uni_w8(bool fire, int nd, unsigned grid, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_uni_w16(bool fire, int nd, unsigned grid, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_fast_w8(bool fire, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_fast_w16(bool fire, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_w8(bool fire, bool lowdim, int cpl, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_w16(bool fire, bool lowdim, int cpl, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);

// a float source quantised in the encoder (quant.h; encode_float_w8.hip / encode_float_w16.hip): the family's kernel of encode_wide.h
// (SPRINTZ_KF_ENC_PAIR with dp lanes a chunk, _ENC_WIDE, _ENC_SPLIT) or the generic one (SPRINTZ_KF_ENC_GENERIC: lowdim, cpl)
hipError_t launch_encode_float_w8(int family, bool fire, bool lowdim, int cpl, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);
hipError_t launch_encode_float_w16(int family, bool fire, bool lowdim, int cpl, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a);

template <typename K, typename A>
inline hipError_t launch_one(K kernel, unsigned grid, size_t shmem, hipStream_t st, const A& a)
{
    if (shmem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), shmem, st, a);
    return hipGetLastError();
}

// (trailing arguments: the kernel template's further parameters -- encode_kernel's FSRC)
#define SPRINTZ_DISPATCH_ENC_T(KERNEL, W, ...)                                                                                    \
    if (lowdim) {                                                                                     \
        if (cpl != 1) return hipErrorInvalidValue;                                                    \
        return fire ? launch_one(KERNEL<W, true, true, 1, ##__VA_ARGS__>, grid, shmem, st, a)                                     \
                    : launch_one(KERNEL<W, false, true, 1, ##__VA_ARGS__>, grid, shmem, st, a);                                   \
    }                                                                                                 \
    switch (cpl) {                                                                                    \
        case 1: return fire ? launch_one(KERNEL<W, true, false, 1, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 1, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 2: return fire ? launch_one(KERNEL<W, true, false, 2, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 2, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 3: return fire ? launch_one(KERNEL<W, true, false, 3, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 3, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 4: return fire ? launch_one(KERNEL<W, true, false, 4, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 4, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 5: return fire ? launch_one(KERNEL<W, true, false, 5, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 5, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 6: return fire ? launch_one(KERNEL<W, true, false, 6, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 6, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        case 8: return fire ? launch_one(KERNEL<W, true, false, 8, ##__VA_ARGS__>, grid, shmem, st, a)                            \
                            : launch_one(KERNEL<W, false, false, 8, ##__VA_ARGS__>, grid, shmem, st, a);                          \
        default: return hipErrorInvalidValue;                                                         \
    }

#define SPRINTZ_DISPATCH_ENC(KERNEL, W) SPRINTZ_DISPATCH_ENC_T(KERNEL, W)

#define SPRINTZ_DISPATCH_Q(KERNEL, W, Q)                                                              \
    if (lowdim) {                                                                                     \
        if (cpl != 1) return hipErrorInvalidValue;                                                    \
        return fire ? launch_one(KERNEL<W, true, true, 1, Q>, grid, shmem, st, a)                     \
                    : launch_one(KERNEL<W, false, true, 1, Q>, grid, shmem, st, a);                   \
    }                                                                                                 \
    switch (cpl) {                                                                                    \
        case 1: return fire ? launch_one(KERNEL<W, true, false, 1, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 1, Q>, grid, shmem, st, a);          \
        case 2: return fire ? launch_one(KERNEL<W, true, false, 2, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 2, Q>, grid, shmem, st, a);          \
        case 3: return fire ? launch_one(KERNEL<W, true, false, 3, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 3, Q>, grid, shmem, st, a);          \
        case 4: return fire ? launch_one(KERNEL<W, true, false, 4, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 4, Q>, grid, shmem, st, a);          \
        case 5: return fire ? launch_one(KERNEL<W, true, false, 5, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 5, Q>, grid, shmem, st, a);          \
        case 6: return fire ? launch_one(KERNEL<W, true, false, 6, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 6, Q>, grid, shmem, st, a);          \
        case 8: return fire ? launch_one(KERNEL<W, true, false, 8, Q>, grid, shmem, st, a)            \
                            : launch_one(KERNEL<W, false, false, 8, Q>, grid, shmem, st, a);          \
        default: return hipErrorInvalidValue;                                                         \
    }

// q: kQueryOff / kQueryMaterialize / kQueryReduceOnly / kQueryWindow (geom.h)
#define SPRINTZ_DISPATCH(KERNEL, W)                                                                   \
    if (q == kQueryOff) { SPRINTZ_DISPATCH_Q(KERNEL, W, kQueryOff) }                                  \
    if (q == kQueryMaterialize) { SPRINTZ_DISPATCH_Q(KERNEL, W, kQueryMaterialize) }                  \
    if (q == kQueryReduceOnly) { SPRINTZ_DISPATCH_Q(KERNEL, W, kQueryReduceOnly) }                    \
    if (q == kQueryWindow) { SPRINTZ_DISPATCH_Q(KERNEL, W, kQueryWindow) }                            \
    return hipErrorInvalidValue;

#define SPRINTZ_FAST_CASE(KERNEL, W, DPV, CPLV, Q, CMV)                                              \
    if (dp == DPV && cpl == CPLV) {                                                                   \
        if (exact) return fire ? launch_one(KERNEL<W, true, DPV, CPLV, true, Q, CMV>, grid, shmem, st, a)  \
                               : launch_one(KERNEL<W, false, DPV, CPLV, true, Q, CMV>, grid, shmem, st, a); \
        return fire ? launch_one(KERNEL<W, true, DPV, CPLV, false, Q, CMV>, grid, shmem, st, a)       \
                    : launch_one(KERNEL<W, false, DPV, CPLV, false, Q, CMV>, grid, shmem, st, a);     \
    }

// decoder fast path: one column per lane for D <= 64, 2 / 4 columns per lane of a
// 64-lane group for D <= 128 / 256
#define SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, Q, CMV)                                             \
    SPRINTZ_FAST_CASE(KERNEL, W, 4, 1, Q, CMV)                                                        \
    SPRINTZ_FAST_CASE(KERNEL, W, 8, 1, Q, CMV)                                                        \
    SPRINTZ_FAST_CASE(KERNEL, W, 16, 1, Q, CMV)                                                       \
    SPRINTZ_FAST_CASE(KERNEL, W, 32, 1, Q, CMV)                                                       \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 1, Q, CMV)                                                       \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 2, Q, CMV)                                                       \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 4, Q, CMV)                                                       \
    return hipErrorInvalidValue;

// the column-major destination exists for the plain decode only (a reduce-only query writes
// no output, so its layout does not matter)
#define SPRINTZ_DISPATCH_DECODE_FAST(KERNEL, W)                                                       \
    if (q == kQueryOff && a.col_stride) { SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, kQueryOff, true) } \
    if (a.col_stride && q == kQueryMaterialize) return hipErrorInvalidValue;                          \
    if (q == kQueryOff) { SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, kQueryOff, false) }               \
    if (q == kQueryMaterialize) { SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, kQueryMaterialize, false) } \
    if (q == kQueryReduceOnly) { SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, kQueryReduceOnly, false) } \
    if (q == kQueryWindow) { SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, kQueryWindow, false) }         \
    return hipErrorInvalidValue;

// every mapping the windowed query has, row-major: the row operations that store no rows (filter, aggregate, histogram, moments, group-by, extrema, linear filter, segments)
#define SPRINTZ_DISPATCH_DECODE_FAST_ROWS(KERNEL, W, Q) SPRINTZ_DISPATCH_DECODE_FAST_Q(KERNEL, W, Q, false)
// gather, select, float rows, rolling rows and cumulative rows: row-major destination, rows of whole 16-byte store pieces -- 16 columns and more, or 8 columns of 16 bits
#define SPRINTZ_FAST_PIECES_8(KERNEL, Q)
#define SPRINTZ_FAST_PIECES_16(KERNEL, Q) SPRINTZ_FAST_CASE(KERNEL, 16, 8, 1, Q, false)
#define SPRINTZ_DISPATCH_DECODE_FAST_PIECES(KERNEL, W, Q)                                             \
    SPRINTZ_FAST_PIECES_##W(KERNEL, Q)                                                                \
    SPRINTZ_FAST_CASE(KERNEL, W, 16, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 32, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 2, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 4, Q, false)                                                     \
    return hipErrorInvalidValue;

// rolling rows, cumulative rows: the one-column-a-lane mappings of the set above, 8 .. 64 columns -- for rolling rows with two and four columns a lane hipcc kept the block's results in
// scratch (tools/kernel_regs.sh), so those shapes stay on the generic kernel (plan.h)
#define SPRINTZ_DISPATCH_DECODE_FAST_PIECES_1(KERNEL, W, Q)                                           \
    SPRINTZ_FAST_PIECES_##W(KERNEL, Q)                                                                \
    SPRINTZ_FAST_CASE(KERNEL, W, 16, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 32, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 1, Q, false)                                                     \
    return hipErrorInvalidValue;

// project rows, derive rows: every one-column-a-lane mapping the plain decode has, 3 .. 64 columns (the projected / derived block, not the row, is what
// must be whole 16-byte pieces: plan.h); two and four columns a lane are not built, those shapes stay on the generic kernel
#define SPRINTZ_DISPATCH_DECODE_FAST_LANES_1(KERNEL, W, Q)                                            \
    SPRINTZ_FAST_CASE(KERNEL, W, 4, 1, Q, false)                                                      \
    SPRINTZ_FAST_CASE(KERNEL, W, 8, 1, Q, false)                                                      \
    SPRINTZ_FAST_CASE(KERNEL, W, 16, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 32, 1, Q, false)                                                     \
    SPRINTZ_FAST_CASE(KERNEL, W, 64, 1, Q, false)                                                     \
    return hipErrorInvalidValue;

// A row operation's translation unit: the instantiations of the generic decoder and of decode_fast for Q, both widths, both codecs.
// The kernels of decode_w8.hip / decode_w16.hip keep the code and the flags they had, and hipcc builds the units in parallel.
// FAST_DISPATCH(KERNEL, W, Q) is the set of decode_fast mappings the mode has.  The generic kernel stages nothing in these modes:
// whatever the plan carved, its launch asks for LDS only where that is the workgroup's table (histogram, group-by) or the chunks' history
// rings (rolling rows, FIR rows) -- and for the filter, which keeps the launch it always had.
#define SPRINTZ_ROW_OP_UNIT(NAME, Q, FAST_DISPATCH)                                                                                                             \
    namespace sprintz {                                                                                                                                         \
    hipError_t decode_generic_##NAME(int w, bool fire, bool lowdim, int cpl, int q, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a)           \
    {                                                                                                                                                           \
        if (q != Q) return hipErrorInvalidValue;                                                                                                                \
        if (Q != kQueryFilter && Q != kQueryHistogram && Q != kQueryGroupBy && Q != kQueryRolling && Q != kQueryFir) shmem = 0;                                                   \
        if (w == 8) { SPRINTZ_DISPATCH_Q(decode_kernel, 8, Q) }                                                                                                 \
        if (w == 16) { SPRINTZ_DISPATCH_Q(decode_kernel, 16, Q) }                                                                                               \
        return hipErrorInvalidValue;                                                                                                                            \
    }                                                                                                                                                           \
    hipError_t decode_fast_##NAME(int w, bool fire, int dp, int cpl, bool exact, int q, int ds, unsigned grid, size_t shmem, hipStream_t st, const DecodeArgs& a) \
    {                                                                                                                                                           \
        if (q != Q || ds != 0 || a.col_stride) return hipErrorInvalidValue;                                                                                     \
        if (w == 16) { FAST_DISPATCH(decode_fast_kernel, 16, Q) }                                                                                               \
        if (w == 8) { FAST_DISPATCH(decode_fast_kernel, 8, Q) }                                                                                                 \
        return hipErrorInvalidValue;                                                                                                                            \
    }                                                                                                                                                           \
    }

#define SPRINTZ_ENC_FAST_CASE(KERNEL, W, DPV, CMV)                                                   \
    case DPV:                                                                                         \
        if (exact) return fire ? launch_one(KERNEL<W, true, DPV, true, CMV>, grid, shmem, st, a)      \
                               : launch_one(KERNEL<W, false, DPV, true, CMV>, grid, shmem, st, a);    \
        return fire ? launch_one(KERNEL<W, true, DPV, false, CMV>, grid, shmem, st, a)                \
                    : launch_one(KERNEL<W, false, DPV, false, CMV>, grid, shmem, st, a);

#define SPRINTZ_DISPATCH_FAST_CM(KERNEL, W, CMV)                                                      \
    switch (dp) {                                                                                     \
        SPRINTZ_ENC_FAST_CASE(KERNEL, W, 4, CMV)                                                      \
        SPRINTZ_ENC_FAST_CASE(KERNEL, W, 8, CMV)                                                      \
        SPRINTZ_ENC_FAST_CASE(KERNEL, W, 16, CMV)                                                     \
        SPRINTZ_ENC_FAST_CASE(KERNEL, W, 32, CMV)                                                     \
        SPRINTZ_ENC_FAST_CASE(KERNEL, W, 64, CMV)                                                     \
        default: return hipErrorInvalidValue;                                                         \
    }

// a.col_stride != 0 selects the column-major source variant
#define SPRINTZ_DISPATCH_FAST(KERNEL, W)                                                              \
    if (a.col_stride) { SPRINTZ_DISPATCH_FAST_CM(KERNEL, W, true) }                                   \
    SPRINTZ_DISPATCH_FAST_CM(KERNEL, W, false)

// a float source's translation unit: the float-source instantiations of encode_wide.h and of the generic encoder for one width
#define SPRINTZ_FLOAT_PAIR_CASE(W, DPV)                                                                                           \
    case DPV:                                                                                                                      \
        if (exact) return fire ? launch_one(encode_wide_float_kernel<W, true, true, false, DPV>, grid, shmem, st, a)               \
                               : launch_one(encode_wide_float_kernel<W, false, true, false, DPV>, grid, shmem, st, a);             \
        return fire ? launch_one(encode_wide_float_kernel<W, true, false, false, DPV>, grid, shmem, st, a)                         \
                    : launch_one(encode_wide_float_kernel<W, false, false, false, DPV>, grid, shmem, st, a);
#define SPRINTZ_FLOAT_SPLIT_8                                                                                                      \
    return fire ? launch_one(encode_wide_float_kernel<8, true, false, true>, grid, shmem, st, a)                                   \
                : launch_one(encode_wide_float_kernel<8, false, false, true>, grid, shmem, st, a);
#define SPRINTZ_FLOAT_SPLIT_16 return hipErrorInvalidValue;      /* (the split mapping is built for 8-bit streams) */
#define SPRINTZ_ENCODE_FLOAT_UNIT(W)                                                                                              \
    namespace sprintz {                                                                                                            \
    hipError_t launch_encode_float_w##W(int family, bool fire, bool lowdim, int cpl, int dp, bool exact, unsigned grid, size_t shmem, hipStream_t st, const EncodeArgs& a) \
    {                                                                                                                              \
        if (a.col_stride || a.norle || a.raw) return hipErrorInvalidValue;                                                         \
        if (family == SPRINTZ_KF_ENC_PAIR) {                                                                                       \
            switch (dp) {                                                                                                          \
                SPRINTZ_FLOAT_PAIR_CASE(W, 4)                                                                                      \
                SPRINTZ_FLOAT_PAIR_CASE(W, 8)                                                                                      \
                SPRINTZ_FLOAT_PAIR_CASE(W, 16)                                                                                     \
                SPRINTZ_FLOAT_PAIR_CASE(W, 32)                                                                                     \
                default: return hipErrorInvalidValue;                                                                              \
            }                                                                                                                      \
        }                                                                                                                          \
        if (family == SPRINTZ_KF_ENC_WIDE) {                                                                                       \
            switch (dp) {                                                                                                          \
                SPRINTZ_FLOAT_PAIR_CASE(W, 64)                                                                                     \
                default: return hipErrorInvalidValue;                                                                              \
            }                                                                                                                      \
        }                                                                                                                          \
        if (family == SPRINTZ_KF_ENC_SPLIT) { SPRINTZ_FLOAT_SPLIT_##W }                                                            \
        if (family != SPRINTZ_KF_ENC_GENERIC) return hipErrorInvalidValue;                                                         \
        SPRINTZ_DISPATCH_ENC_T(encode_kernel, W, true)                                                                            \
    }                                                                                                                              \
    }

}  // namespace sprintz
