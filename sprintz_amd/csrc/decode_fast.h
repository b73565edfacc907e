// decode_fast.h -- the decoder the headline benchmark runs (general row-major
// payload layout, one column per lane, D <= 64): an LDS-staged, prefetching,
// instruction-lean version of decode_kernel.h with identical stream semantics
// (sprintz_xff_rle.cpp:569-1179, sprintz_delta_rle.cpp:418-772).
//
// What bounded the first two versions (profiles/r1_*): ~10 global-load
// wave-instructions per 8-row block, each carrying 64 scattered 4-byte
// requests over 8 streams (~30 cycles of texture-addresser time apiece), and
// two dependent HBM/L2 round trips per block.  Here instead:
//   * INPUT.  A group (DP lanes = one chunk) reads its compressed stream
//     strictly sequentially, so it is read AHEAD of the parser: one 16-byte
//     global load per lane per refill (DP*16 = one "unit") is issued a whole
//     group (16 rows) before its bytes are parsed and parked in a per-group LDS
//     ring of 6 units (+ an apron that mirrors the ring head, so that a group's
//     reads never wrap).  Headers, run lengths and bit fields are then LDS reads
//     (aligned ds_read2_b32 + v_alignbyte_b32) -- no global load sits on the
//     parse critical path.  Units are whole cache lines: the read-ahead starts
//     on the 128-byte line the stream starts in, so that a unit is ONE line per
//     group and load instruction and no line is asked for by two of them.
//   * FIELDS. rows are byte aligned, so the in-byte shift of a column is the
//     same for all 8 rows: field = v_bfe_u32(dword at row base, shift, nbits).
//   * FIRE.   with E = err << W:  delta = sbfe((prev_delta*coef + E), W, W)
//     == sext_W(err + ((prev_delta*coef) >> W)) exactly, W-bit wrap included
//     (the low W bits of the product cannot carry into a multiple of 2^W);
//     sign(err) for the coefficient gradient is one v_med3_i32.
//   * HEADER. both slots' nbits ride in one register through a DPP scan.
//   * OUTPUT. the 8 x D block is transposed through LDS, leaves as dwordx4.
#pragma once

#include <type_traits>

#include "decode_kernel.h"
#include "group_ops.h"

namespace sprintz {

typedef uint32_t __attribute__((aligned(1), may_alias)) u32_unaligned;
struct __attribute__((aligned(1), packed)) u128_unaligned { uint32_t x, y, z, w; };

typedef __attribute__((address_space(3))) const uint32_t lds_u32;
typedef __attribute__((address_space(3))) const uint8_t lds_u8;

// 32 bits at ANY byte address `a` of LDS.  gfx950 replays a misaligned
// ds_read_b32 (SQ_LDS_UNALIGNED_STALL: it made the first ring version 1.7x
// slower than the global-load kernel), so: one aligned ds_read2_b32 +
// v_alignbyte_b32, which takes the byte phase straight from the low two address
// bits (verified on hardware, tools/probes/alignbyte.hip).
__device__ __forceinline__ uint32_t lds_rd32(uint32_t a)
{
    lds_u32* q = (lds_u32*)(uintptr_t)(a & ~3u);
    return __builtin_amdgcn_alignbyte(q[1], q[0], a);
}
__device__ __forceinline__ uint32_t lds_rd8(uint32_t a) { return *(lds_u8*)(uintptr_t)a; }
__device__ __forceinline__ uint32_t lds_addr(const void* p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// a 64-bit value that is the same in every lane of the wavefront, moved to SGPRs
// (the builtin returns int: go through uint32_t, or a low word >= 2^31 sign-extends into the high one)
__device__ __forceinline__ uint64_t wave_uniform64(uint64_t x)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// 24-bit multiply-add / multiply, pinned to the full-rate opcodes (hipcc turns
// __mul24 of values it cannot range-prove into quarter-rate v_mul_lo_u32)
__device__ __forceinline__ int mad24(int a, int b, int c)
{
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// sign(x) in {-1, 0, 1} = clamp(x, -1, 1): one v_med3_i32 (hipcc lowers the C++
// min/max form to two cmp+cndmask pairs)
__device__ __forceinline__ int sign_of(int x)
{
    int s;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(s) : "v"(x));
    return s;
}

// 16-bit FIRE step without the shift: D = (i16)hi16(a) * (i16)b + c.  With X = prev_delta*coef + E
// the new delta IS the high half of X, so the recurrence feeds X straight back in
// (verified against the C model and timed at full rate on hardware: tools/probes/mad_i16.hip).
__device__ __forceinline__ int mad_i16_hi(int a, int b, int c)
{
    int d;
    asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// a + hi16(x): the running value only matters modulo 2^16, so the unsigned high half will do
__device__ __forceinline__ uint32_t add_hi16(uint32_t a, int x)
{
    uint32_t d;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(d) : "v"(a), "v"(x));
    return d;
}

// CPL columns per lane (column = lane_d*CPL + k); EXACT: ndims == DP*CPL, so every
// size is a compile-time constant.
// CM: column-major destination (DecodeArgs::col_stride): the 8 samples a lane produces per block
// are contiguous in ITS column -- packed in registers and stored as one 16-byte (8-byte at
// W == 8) piece per column, no LDS transpose.
// DS != 0: the LDS carve (ring, apron, requests per step) is sized for streams of at most DS columns instead of the
// DP*CPL the lanes could hold (the launch checks ndims <= DS) -- what decides how many chunks a CU keeps in flight.
// CPL == 3 is the SPLIT mapping for 8-bit streams of 65 .. 96 columns on 32 lanes (two chunks a wavefront instead of one
// on 64 x 2 with 40 lanes busy at 80 columns): lane l owns the PAIR (2l, 2l+1) -- every pair genuine, on an even column,
// so the paired window / paired staging write of the 8-bit path apply -- and the SINGLE column 64 + l.
template <int W, bool FIRE, int DP, int CPL, bool EXACT, int Q = 0, bool CM = false, int DS = 0>
__global__ void __launch_bounds__(kThreads) decode_fast_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t v4u;
    constexpr int HB = Elem<W>::HB;
    constexpr int ESZ = W / 8;
    constexpr int LOG2DP = DP == 4 ? 2 : DP == 8 ? 3 : DP == 16 ? 4 : DP == 32 ? 5 : 6;
    constexpr int DCAP = DP * CPL;                         // columns a group can hold
    constexpr uint32_t ROW16 = DP * 16;                    // bytes one wave-instruction moves per group
    constexpr uint32_t UNIT = ROW16 * CPL;                 // bytes one refill unit brings in (CPL pieces per lane)
    constexpr bool SPLIT = CPL == 3;
    static_assert(!SPLIT || (W == 8 && DP == 32 && !EXACT && !CM && Q == 0), "the split mapping is built for 8-bit row-major decodes");
    // GATHER (sprintz_mi355x_gather_rows): a lane group decodes ONE piece -- rows [lo, hi) of one chunk, for one range -- from the chunk's
    // row 0, stores those rows alone and stops after row hi - 1.  The groups of a wave then work on unrelated chunks and unrelated output
    // rows: both descriptors are based at the container / at `out` (the launch checks that both spans fit 32-bit offsets), and the
    // launch takes only rows of whole 16-byte pieces, so that a store piece lies in ONE row and the row test decides it as a whole.
    constexpr bool GATHER = Q == kQueryGather;
    static_assert(!GATHER || (!CM && !SPLIT && DS == 0), "gather: row-major destination, plain mappings");
    // SELECT (sprintz_mi355x_select_rows): a plain decode of the group's chunks whose store pieces go, row by row, where the caller's mask
    // and the chunk's base send them -- or nowhere.  The chunks of a wave land in unrelated output rows: the store descriptor is based
    // at `out` and spans its select.capacity rows (the launch checks that they fit 32-bit offsets), and, as for the gather, the launch takes
    // only rows of whole 16-byte pieces.
    constexpr bool SELECT = Q == kQuerySelect;
    static_assert(!SELECT || (!CM && !SPLIT && DS == 0), "select: row-major destination, plain mappings");
    // AGGREGATE (sprintz_mi355x_aggregate_rows): the windowed query over the rows the caller's mask names.  Nothing is stored but the
    // windows' entries, so any shape the windowed query takes is taken; the mask bytes come through select's read-ahead window.
    constexpr bool AGG = Q == kQueryAggregate;
    static_assert(!AGG || (!CM && !SPLIT && DS == 0), "aggregate: plain mappings");
    // HIST (sprintz_mi355x_histogram_rows): per-column value counts of the rows the caller's mask names (or of every row).  Nothing is
    // stored: the samples are counted in the workgroup's LDS table behind the groups' carves (decode_ops.h: hist_begin .. hist_end); the
    // mask bytes come through select's read-ahead window.  The workgroup's lanes meet at two barriers, so no lane leaves early.
    constexpr bool HIST = Q == kQueryHistogram;
    static_assert(!HIST || (!CM && !SPLIT && DS == 0), "histogram: plain mappings");
    // MOM (sprintz_mi355x_moments_rows): per window the number of rows the caller's mask names (or of every row) and per column their
    // sum, sum of squares and sum of products with ONE reference column.  That column is decoded in one slot of one lane, so a lane
    // keeps the block's rows of all its slots and forms the products behind the slot loop, when the reference lane can hand its 8
    // rows over (decode_ops.h: moments_ref_rows).  Windows, mask read-ahead and run shortcut are aggregate's.
    constexpr bool MOM = Q == kQueryMoments;
    static_assert(!MOM || (!CM && !SPLIT && DS == 0), "moments: plain mappings");
    // GBY (sprintz_mi355x_groupby_rows): per bin of ONE key column's value, the count and the per-column sums of the rows the caller's mask
    // names (or of every row).  Where a sample is added depends on another column's value: a lane keeps the block's rows of all its slots,
    // as the moments do, until the key column's lane has handed its 8 rows over; the entries are added up in the workgroup's LDS table
    // behind the groups' carves (decode_ops.h: groupby_begin .. groupby_end), so, as for the histogram, no lane leaves early.
    constexpr bool GBY = Q == kQueryGroupBy;
    static_assert(!GBY || (!CM && !SPLIT && DS == 0), "group-by: plain mappings");
    // EXT (sprintz_mi355x_extrema_rows): per window and column the minimum and the maximum of the rows the caller's mask names (or of every
    // row) with the rows they stand in, the column's value in the window's first and last selected row, those two rows and the count.
    // Windows, mask read-ahead and the shape of the run shortcut are aggregate's; value and row stay apart (decode_ops.h: ExtremaAcc).
    constexpr bool EXT = Q == kQueryExtrema;
    static_assert(!EXT || (!CM && !SPLIT && DS == 0), "extrema: plain mappings");
    // LIN (sprintz_mi355x_filter_linear): the filter's outputs -- a mask byte a block, the chunk's count -- for a predicate on a linear form
    // over the row and the row in front of it.  A lane adds its columns' terms into the block's eight partial sums, the group adds those up
    // once a block (decode_ops.h: linear_rows8, linear_block).
    constexpr bool LIN = Q == kQueryLinear;
    static_assert(!LIN || (!CM && !SPLIT && DS == 0), "linear filter: plain mappings");
    // SEG (sprintz_mi355x_segment_rows): aggregate's accumulators over windows whose edges come from the caller's mask -- a run of set bits, or
    // the stretch between two of them -- placed as select places rows, behind the chunk's base (decode_ops.h: SegState, segment_rows8).
    // Nothing is stored but the segments' entries; mask read-ahead and the column's 8 waiting rows are aggregate's.
    constexpr bool SEG = Q == kQuerySegment;
    static_assert(!SEG || (!CM && !SPLIT && DS == 0), "segments: plain mappings");
    // FLT (sprintz_mi355x_float_rows): a plain decode whose store pieces convert.  Staging and held[][] stay in the element type -- the LDS
    // carve and the registers a block waits in are the plain decode's -- and a piece becomes float32 / float16 / bfloat16 where it is stored:
    // 16 input bytes leave as OSZ / ESZ 16-byte stores.  The launch takes only rows of whole 16-byte INPUT pieces, so a lane's piece q holds the
    // same columns in every block and their scales and offsets are loaded once (fsc / fof).  Everything counted in output bytes -- the
    // descriptor's base and span, the cursor ovo -- uses the output element's size OSZ, not ESZ.
    constexpr bool FLT = Q == kQueryFloat;
    static_assert(!FLT || (!CM && !SPLIT && DS == 0), "float rows: row-major destination, plain mappings");
    // ROLL (sprintz_mi355x_rolling_rows): nothing of the raw block is stored.  A column's 8 rows wait in arow for q_block, which runs the rolling
    // step on the chunk's history ring -- behind the groups' carves, at a.table.table_off -- and keeps the block's results in registers (rres);
    // behind the columns roll_out sends them through the plain decode's staging, one plane at a time, and out as 16-byte pieces: the minima and
    // the maxima as element-type planes to their own outputs, the sum as 32 / W element-type planes (its bytes, low first) that are joined into
    // 32-bit pieces where float rows convert theirs.  The pieces are stored at once (no held slots: three outputs would triple them).
    constexpr bool ROLL = Q == kQueryRolling;
    static_assert(!ROLL || (!CM && !SPLIT && DS == 0 && CPL == 1), "rolling rows: row-major destination, one column a lane (with 2 and 4 hipcc put the block's results in scratch)");
    // PROJ (sprintz_mi355x_project_rows): a plain decode, or float rows, whose staged block holds only the K columns a slot table names.  A lane
    // loads its column's slot once; a selected column is staged at slot * ESZ of rows of K * ESZ bytes, an unselected one at a spare place behind
    // the projected block that no piece reads.  Every output-byte quantity -- row_stride, blk_bytes, the chunk's base in the descriptor, the
    // descriptor's span, the tail -- counts K columns; blk_elems and out_left keep counting all D, as the stream and d_rets do.  The projected
    // block is a whole number of 16-byte pieces (the launch checks), a projected ROW need not be: a piece may wrap from one row into the next, so
    // the scale and the offset of its element j are slot (c0 + j) % K's.  Unconverted or converted is a wave-uniform switch (filter.mode).
    constexpr bool PROJ = Q == kQueryProject;
    static_assert(!PROJ || (!CM && !SPLIT && DS == 0 && CPL == 1), "project rows: row-major destination, one column a lane");
    // CUM (sprintz_mi355x_cumulative_rows): nothing of the raw block is stored.  A column's 8 rows wait in arow for q_block, which runs the running
    // min / max / sum on (decode_ops.h: cumulative_step8) and keeps the block's results in registers (rres: the minima, the maxima, the sums' low
    // and high words); behind the columns cum_out sends them through the plain decode's staging a plane at a time, as rolling rows do: the minima
    // and the maxima as element-type planes to their own outputs, the sums sum_bytes / ESZ times the block's bytes, a quarter or an eighth of the
    // block's rows at a pass.  No LDS of its own, and no barrier the plain decode has not.
    constexpr bool CUM = Q == kQueryCumulative;
    static_assert(!CUM || (!CM && !SPLIT && DS == 0 && CPL == 1), "cumulative rows: row-major destination, one column a lane");
    // DER (sprintz_mi355x_derive_rows): nothing of the raw block is stored or staged.  A column's 8 rows wait in arow for der_out, behind the column:
    // a form at a time, the lane multiplies its rows (and the rows in front of them: dlast hands row 7 over the block seam) by its column's two weights
    // -- read from the workgroup's table in LDS, [K][D] pairs at a.table.table_off, filled once at the kernel's start -- the group adds the 8 partial
    // sums up (group_add), and lane i mod DP puts row i's value, converted or not, at its place of the derived block in the group's staging: 8 rows
    // of K values, in output order.  The block then leaves as whole 16-byte pieces, stored at once as rolling rows' are.  Every output-byte quantity
    // -- the chunk's base in the descriptor, the descriptor's span, the cursor ovo -- counts K values of OSZ bytes a row; the launch sizes the staging
    // for 8 K OSZ bytes where that is more than the decoded block (plan.h).
    constexpr bool DER = Q == kQueryDerive;
    static_assert(!DER || (!CM && !SPLIT && DS == 0 && CPL == 1), "derive rows: row-major destination, one column a lane");
    // FIR (sprintz_mi355x_fir_rows): nothing of the raw block is stored.  A column's 8 rows wait in arow for q_block, which runs the filter step on the
    // chunk's history ring -- rolling rows' ring, behind the groups' carves at a.table.table_off -- with the column's taps from the workgroup's table in
    // LDS ([T][D] int32 behind the rings, filled once at the kernel's start), converts where a float format is asked and keeps the block's 8 results in
    // registers (rres); behind the columns fir_out sends them through the plain decode's staging AS OUTPUT ELEMENTS, in output order, 8 ESZ / OSZ rows
    // of the block at a pass, and out as 16-byte pieces, as cumulative rows' sums leave.  The pieces are stored at once.
    constexpr bool FIR = Q == kQueryFir;
    static_assert(!FIR || (!CM && !SPLIT && DS == 0 && CPL == 1), "FIR rows: row-major destination, one column a lane");
    // the modes that take the rows a mask names (decode_ops.h: RowMaskArgs); all but select, aggregate and segments take a null mask for "every row"
    constexpr bool MASKED = SELECT || AGG || HIST || MOM || GBY || EXT || SEG;
    constexpr bool MASK_GIVEN = SELECT || AGG || SEG;      // (no test for a null mask where there always is one: select measured 1 % slower with it)
    constexpr int DSZ = DS ? DS : DCAP;                    // columns the LDS carve is sized for
    static_assert(DSZ <= DCAP, "sizing columns");
    constexpr uint32_t HDRMAX = (2 * DSZ * HB + 7) / 8;
    constexpr uint32_t BLKMAX = 8 * DSZ * ESZ;             // largest block payload = largest decoded block
    constexpr int PIECES = (BLKMAX + ROW16 - 1) / ROW16;   // 16-byte pieces of a decoded block per lane
    constexpr uint32_t CG = HDRMAX + 2 * BLKMAX + 4;       // most bytes one group can consume
    constexpr uint32_t NPEND = (CG + UNIT - 1) / UNIT;     // units requested per group step (2 or 3)
    constexpr uint32_t CSTART = 16 + 8;                    // chunk start: alignment gap + 8-byte stream header
    // (a ring of 4 units instead of 6 -- 960 bytes a group, 20 waves a CU instead of 16, safe only for compressible
    //  streams -- was timed on the headline batch: 0.4124 -> 0.4079 ms.  Occupancy is not what holds this kernel.)
    constexpr uint32_t RBU = (2 * (CG + CSTART) + 3 + UNIT - 1) / UNIT + 1;   // ring units: 6 @16 bit, 4 @8 bit
    constexpr uint32_t RB = RBU * UNIT;                    // ring bytes
    constexpr uint32_t APRON = (CG + CSTART + 8 + 15) & ~15u;   // a step never reads past its start + APRON
    static_assert(RB - UNIT >= 2 * (CG + CSTART) + 3, "ring too small for one step of read-ahead");
    static_assert(NPEND <= 3, "pending registers");
    // A read-ahead (re)starts on a cache line: the ABSOLUTE address of a group's first unit is rounded down to LINE, so that
    // a unit -- 128 contiguous bytes per group and load instruction where it is that long -- lies in one line instead of two.
    // The parse cursor then starts up to LINE - 1 bytes into the ring, which the prime has to leave room for.
    constexpr uint32_t LINE = UNIT >= 128u ? 128u : UNIT;
    static_assert((LINE & (LINE - 1)) == 0 && LINE >= 16, "line phase is a mask");
    static_assert(RB - (LINE - 1) >= CG + CSTART, "ring too small for the first step after a line-aligned prime");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int D = EXACT ? DCAP : a.D;
    const uint64_t gtid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane_d = (int)(threadIdx.x & (uint32_t)(DP - 1));
    // A group decodes `chunks_per_group` CONSECUTIVE chunks.  Their streams are
    // (nearly) contiguous in the container, so the ring's read-ahead runs straight
    // across chunk boundaries: one cold start per group instead of one per chunk.
    GatherPiece gp{};
    uint64_t c_sel = (gtid >> LOG2DP) * (uint64_t)a.chunks_per_group;
    if constexpr (GATHER) {                                // consecutive piece slots on consecutive groups: a range's chunks share a wave
        if (!gather_piece(a, gtid >> LOG2DP, gp)) return;
        // (a stream that 32-bit offsets cannot reach: the launch's size bound holds for every container the library writes)
        if (gp.exists && a.offsets[gp.chunk + 1] > 0xfffffff0ull - 4096u) { if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt); return; }
        if (!gp.exists) { if (lane_d == 0) gather_fail(a, gp.range, kErrNoRow); return; }
        c_sel = gp.chunk;
    }
    const uint64_t c_first = c_sel;
    if constexpr (DER) {                                   // the workgroup's table of weights, every lane of it, before any leaves
        uint2* const wt = (uint2*)(smem + a.table.table_off);
        const uint32_t n = derive_k(a) * (uint32_t)D;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) wt[i] = make_uint2((uint32_t)a.lin.w[i], a.lin.lag ? (uint32_t)a.lin.lag[i] : 0u);
        __syncthreads();
    }
    if constexpr (FIR) {                                   // the workgroup's table of taps, every lane of it, before any leaves
        uint32_t* const tt = (uint32_t*)(smem + a.table.table_off + (size_t)(kThreads >> LOG2DP) * (size_t)roll_ring_bytes(a.win.rows, D, ESZ));
        const uint32_t n = fir_ntaps(a) * (uint32_t)D;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) tt[i] = (uint32_t)a.lin.w[i];
        __syncthreads();
    }
    if constexpr (!HIST && !GBY) {
        if (c_first >= a.nchunks) return;
    }                                                      // (histogram, group-by: c_end <= c_first below, and the chunk loop does not run)
    const uint64_t c_end = GATHER ? c_first + 1 : (c_first + a.chunks_per_group < a.nchunks) ? c_first + a.chunks_per_group : a.nchunks;

    // LDS carve per group: [ring RB | apron APRON | block staging]
    uint8_t* const ringp = smem + (size_t)(threadIdx.x >> LOG2DP) * a.lds_group_stride;
    const uint32_t ring = lds_addr(ringp);                 // LDS byte address of the ring
    uint8_t* const stage = ringp + RB + APRON;
    // rolling rows: the chunk's history ring (decode_ops.h: rolling_ring), a ring a group behind every group's carve
    uint8_t* rollp = nullptr;
    if constexpr (ROLL || FIR) rollp = smem + a.table.table_off + (size_t)(threadIdx.x >> LOG2DP) * (size_t)roll_ring_bytes(a.win.rows, D, ESZ);

    // stream geometry.  All stream loads go through ONE wave-uniform buffer
    // descriptor that spans the container from this wavefront's first stream to its
    // end: offsets are 32-bit, and a load that runs past the container returns 0
    // instead of faulting -- the read-ahead needs no bounds test.
    const uint64_t wave_first = GATHER ? 0 : (((uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u)) >> LOG2DP) * (uint64_t)a.chunks_per_group;
    // The descriptor starts on the cache line of the wave's first stream -- unless that line starts in front of the
    // container (a first stream less than LINE bytes into a container that is not line-aligned): no address below a.comp
    // is ever formed, and such a wave keeps the 16-byte rule.  Every load address is base + offset with offset >= 0.
    const uint32_t comp_lo = (uint32_t)(uintptr_t)a.comp;
    uint64_t wave_base = 0;
    if constexpr (!GATHER) {
        const uint64_t off0 = a.offsets[wave_first < a.nchunks ? wave_first : 0];
        const uint32_t ph0 = (comp_lo + (uint32_t)off0) & (LINE - 1);
        wave_base = ph0 <= off0 ? off0 - ph0 : off0 & ~(uint64_t)15;
        wave_base = wave_uniform64(wave_base);
    }
    // 15 bytes past the last stream, so that the 16-byte piece holding its last byte ends in range whatever the piece's
    // phase (gfx950 zeroes a dwordx4 whose END is out of range); they are inside the SPRINTZ_MI355X_READ_SLACK the API asks for
    const uint64_t wave_span = (a.offsets[a.nchunks] - wave_base) + 15;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.comp + wave_base), 0, (uint32_t)(wave_span < 0xffffffffull ? wave_span : 0xffffffffull), 0x00020000);
    // output: one descriptor per wave as well, based at its first chunk's slot; a store
    // whose offset is out of range is dropped by the hardware, which is what the
    // unconditional per-step block stores rely on before a lane has produced a block
    // (column-major: the descriptor starts at this wave's first ROW of column 0 and runs to the
    //  end of the last column; offsets are column*col_stride + row, in bytes)
    const uint32_t rows_per_chunk = CM ? a.chunk_len / (uint32_t)(EXACT ? DCAP : a.D) : 0u;
    // float rows: the output element's bytes, and the shift that turns a byte offset among decoded elements into one among converted ones
    // (project rows: the same two, with the element type itself as one more format -- pflt: the pieces convert; and the elements of a chunk's
    //  projected slot, R x K)
    const bool pflt = PROJ && !(a.filter.mode & kProjectRawBit);
    const uint32_t OSZ = FLT ? (uint32_t)float_out_bytes(a.filter.mode) : PROJ ? (uint32_t)project_out_bytes(a.filter.mode, ESZ)
                       : DER ? (uint32_t)derive_out_bytes(a.filter.mode) : (uint32_t)ESZ;
    const uint32_t fshift = FLT ? (OSZ == 4u ? (ESZ == 1 ? 2u : 1u) : (ESZ == 1 ? 1u : 0u))
                          : PROJ ? (OSZ == 4u ? (ESZ == 1 ? 2u : 1u) : (OSZ == 2u && ESZ == 1 ? 1u : 0u)) : 0u;
    // (derive rows: K and the elements of a chunk's derived slot, R x K, in the same two)
    const uint32_t pK = PROJ ? project_k(a) : DER ? derive_k(a) : 0u;
    const uint32_t pslot_elems = (PROJ || DER) ? a.chunk_len / (uint32_t)(EXACT ? DCAP : a.D) * pK : 0u;
    const uint64_t out_base = (PROJ || DER) ? (wave_first < a.nchunks ? wave_first : 0) * (uint64_t)pslot_elems * OSZ
                            : FLT ? (wave_first < a.nchunks ? wave_first : 0) * (uint64_t)a.chunk_len * OSZ
                            : CM ? (wave_first < a.nchunks ? wave_first : 0) * (uint64_t)rows_per_chunk * ESZ
                            : SELECT ? 0
                                 : (wave_first < a.nchunks ? wave_first : 0) * (uint64_t)a.chunk_len * ESZ;
    const uint64_t out_span = (PROJ || DER) ? a.nchunks * (uint64_t)pslot_elems * OSZ - out_base
                            : FLT ? a.nchunks * (uint64_t)a.chunk_len * OSZ - out_base
                            : CM ? (uint64_t)(EXACT ? DCAP : a.D) * a.col_stride * ESZ - out_base
                            : GATHER ? a.gather.nranges * (uint64_t)a.gather.rows * (uint64_t)(EXACT ? DCAP : a.D) * ESZ
                            : SELECT ? a.select.capacity * (uint64_t)(EXACT ? DCAP : a.D) * ESZ
                                 : a.nchunks * (uint64_t)a.chunk_len * ESZ - out_base;
    // (both are wave-uniform by construction; saying so keeps hipcc from wrapping every store in a
    //  readfirstlane waterfall loop -- 8 VALU per store it cannot prove away)
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((uint8_t*)a.out + wave_uniform64(out_base)), 0,
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(out_span < 0xfffffff0ull ? out_span : 0xfffffff0ull)), 0x00020000);
    constexpr uint32_t kDropStore = 0xfffffff0u;          // out of range of every descriptor
    // the decoded samples are written once and not read again by this kernel: non-temporal stores (aux bit 1 = nt)
    // keep them from displacing the compressed streams in L2 and let whole lines go out -- measured with the
    // univariate decoder first (0.402 -> 0.336 ms on BASELINE config 1)
#ifndef SPRINTZ_STORE_AUX
#define SPRINTZ_STORE_AUX 2
#endif
#ifndef SPRINTZ_DF_MERGE8
#define SPRINTZ_DF_MERGE8 1
#endif
    constexpr int kStoreAux = SPRINTZ_STORE_AUX;
    const uint32_t lane16 = (uint32_t)lane_d * 16u;
    uint64_t gabs = 0;                                     // container offset the cursors below are relative to
    uint32_t gvo = 0;                                      // this lane's next 16 bytes to request (offset from wave_base)
    uint32_t rp = 0;                                       // parse cursor (offset from gabs)
    uint32_t rofs = 0;                                     // parse cursor (ring offset)
    uint32_t ahead = 0;                                    // bytes requested and not yet parsed
    uint32_t cofs = lane16;                                // ring offset where this lane parks its next 16 bytes

    uint4 pend[3][CPL];
    uint32_t npend = 0;

    // Request one unit (CPL 16-byte pieces per lane).  The loads are UNCONDITIONAL (an
    // unwanted unit asks for an offset outside the descriptor) so that the compiler can count
    // the VMEM operations of a step exactly -- see the wait discussion at the bottom of the loop.
    auto request = [&](uint4 (&v)[CPL], bool wanted) {
#pragma unroll
        for (int j = 0; j < CPL; j++) {
                        // (non-temporal LOADS were tried too: the read-ahead re-reads what neighbouring groups fetched, and with nt
            //  those re-reads go back to HBM -- 0.413 -> 0.461 ms)
            // an unwanted unit asks for an offset outside the descriptor: the texture addresser answers zeros without a request to
            // the cache (a re-read of offset 0 is a real request of 64 lanes, and the addresser's queue is what the block stores wait in)
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, wanted ? gvo + j * ROW16 : 0xfffffff0u, 0, 0);
            v[j] = make_uint4(t[0], t[1], t[2], t[3]);
        }
        gvo += wanted ? UNIT : 0u;
    };
    auto commit = [&](const uint4 (&v)[CPL]) {             // park one unit in the ring (+ mirror the ring head)
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            const uint32_t ro = cofs + j * ROW16;
            *(uint4*)(ringp + ro) = v[j];
            if (ro < APRON) *(uint4*)(ringp + RB + ro) = v[j];
        }
        cofs += UNIT;
        if (cofs >= RB) cofs -= RB;
    };
    // (re)start the read-ahead at container offset `off`: fill the whole ring, from the cache line `off` lies in.
    // (Where that line starts in front of the descriptor -- only a wave under the 16-byte rule above, or a gather piece in
    //  the container's first line -- from the 16-byte piece instead: off & ~15 >= wave_base, which is a multiple of 16 there.)
    auto prime = [&](uint64_t off) {
        const uint32_t ph = (comp_lo + (uint32_t)off) & (LINE - 1);
        gabs = ph <= off - wave_base ? off - ph : off & ~(uint64_t)15;
        gvo = (uint32_t)(gabs - wave_base) + lane16;
        rp = (uint32_t)(off - gabs);
        rofs = rp;
        cofs = lane16;
        npend = 0;
        wave_lds_sync();
#pragma unroll
        for (uint32_t u = 0; u < RB / UNIT; u++) {
            uint4 v[CPL];
            request(v, true);
            commit(v);
        }
        ahead = RB - rp;
        wave_lds_sync();
    };

    const uint32_t hdr_bytes = (2u * (uint32_t)D * HB + 7u) >> 3;
    const uint32_t blk_elems = 8u * (uint32_t)D;
    const uint32_t blk_bytes = PROJ ? 8u * pK * ESZ : blk_elems * ESZ;      // (project rows: the bytes of a staged, projected block and of its rows)
    const uint32_t row_stride = PROJ ? pK * ESZ : (uint32_t)D * ESZ;
    const int col0 = lane_d * CPL;                         // first column of this lane
    // A lane column past the last one (ndims is not DP*CPL) stands in for column D-1: it reads the same header fields and
    // bit fields, runs the same recurrence and stages the same bytes at the same place as the genuine one -- so the per-sample
    // code needs no predicate (54 exec-mask regions a group step at 80 columns on 64 x 2); only the scan must not count it.
    // (8 bits, an even number of columns per lane, row-major output: a lane's two ADJACENT columns leave as one 16-bit staging
    //  write per row -- half the ds_write instructions, which is what bounds this shape (4 LDS cycles per ds_write_b8, 2 per
    //  sample for the field window).  A lane past the last column then stands in for the last PAIR, (D-2, D-1) -- the same two
    //  bytes at the same address as the genuine lane's; with an odd D the last lane's second byte spills into the next row's
    //  first, which that row's own write -- DS operations of a wave execute in order -- puts right, and after row 7 into padding.)
    constexpr bool MERGE8 = SPRINTZ_DF_MERGE8 && W == 8 && (CPL % 2 == 0 || SPLIT) && !CM && Q == 0;
    const bool merge8 = MERGE8 && (EXACT || (D & 1) == 0);   // rows of an odd number of bytes would make every second 16-bit write misaligned
    constexpr int NPAIR = CPL / 2;                         // columns 2j, 2j+1 (j < NPAIR) of a lane are adjacent in the row
    int genk[CPL];                                         // the column this lane column IS (>= D: it is a stand-in)
    int colk[CPL];
    uint8_t* stage_k[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        genk[k] = SPLIT ? (k < 2 ? 2 * lane_d + k : 2 * DP + lane_d) : col0 + k;
        if (MERGE8 && merge8 && !SPLIT) {
            const int pb = (col0 + (k & ~1)) < D ? col0 + (k & ~1) : ((D - 1) & ~1);      // first column of this lane's pair
            colk[k] = EXACT ? col0 + k : (pb + (k & 1) < D ? pb + (k & 1) : D - 1);
        } else {
            colk[k] = EXACT ? genk[k] : (genk[k] < D ? genk[k] : D - 1);
        }
        stage_k[k] = stage + colk[k] * ESZ;
    }
    // project rows: the lane's slot (a stand-in lane takes its genuine twin's: the same bytes at the same place) and the stride of its staged rows
    // -- 0 for a column that is not selected, whose 8 samples all go to the spare bytes behind the projected block (8 K ESZ <= 8 D ESZ, and the
    // carve ends 16 bytes behind that: geom.h, decode_fast_lds_bytes)
    uint32_t prs = 0;
    if constexpr (PROJ) {
        const uint32_t sl = (uint32_t)project_slot(a, (uint32_t)colk[0]);
        const bool psel = sl < pK;
        prs = psel ? row_stride : 0u;
        stage_k[0] = stage + (psel ? sl * ESZ : blk_bytes);
    }

    uint32_t pv[CPL];
    int pd[CPL], ctr[CPL];
    bool col_ok[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) { pv[k] = 0; pd[k] = 0; ctr[k] = 0; col_ok[k] = EXACT ? true : genk[k] < D; }
    uint32_t out_left = 0;                                 // capacity guard (elements)
    bool corrupt = false;
    // query-on-compressed (Q != 0): per-column max and sum of the chunk, kept next to the
    // predictor state; with Q == kQueryReduceOnly the block never leaves the registers
    uint32_t qmax[CPL];
    uint64_t qsum[CPL];
    uint32_t qbs[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) { qmax[k] = 0; qsum[k] = 0; qbs[k] = 0; }
    // windowed query (Q == kQueryWindow): the minimum too, and the chunk's window being accumulated with the rows it
    // still takes; a window's entries leave with the block that completes it (blocks never straddle a window edge)
    constexpr uint32_t MASK = Elem<W>::MASK;
    uint32_t qmin[CPL];                                    // (set at each chunk start, in that mode alone)
    uint32_t wi = 0, wleft = 0;
    uint64_t wbase = 0;
    // filter rows (Q == kQueryFilter): this lane's columns' bounds, loaded once; fcm collects the 8 rows of the column being decoded,
    // fl the lane's columns (inverted domain: decode_ops.h, FilterCol); the group ORs its lanes once per block (f_block)
    FilterCol fc[CPL];
    uint32_t finv = 0, fcm = 0, fl = 0, fb = 0, fcnt = 0;  // fb: blocks of this chunk done = the mask byte the next block writes
    // select / aggregate rows: the mask byte of the block being decoded (fb counts the chunk's blocks, as for the filter); aggregate: the
    // rows of the column being decoded and the selected rows of the window so far
    uint32_t sm = 0;
    uint32_t arow[8];
    uint32_t acnt = 0;
    uint8_t* fmb = nullptr;
    // segment rows: the group's walk over its chunk's segments, the block being decoded under the rule, the chunk's base and its first batch
    // row; seg_loop: some group of the wavefront has a start or an end in its block, so all of them walk their block's rows (wave-uniform)
    SegState sst{0, 0, 0};
    SegBlock sblk{0, 0, 0};
    uint64_t gbase = 0, grow0 = 0;
    bool seg_loop = false;
    // moments rows: the block's rows of every slot of the lane, and the lane's accumulators (acnt: the window's selected rows)
    uint32_t mrow[CPL][8];
    MomentAcc macc[CPL];
    if constexpr (MOM) {
#pragma unroll
        for (int k = 0; k < CPL; k++) macc[k] = MomentAcc{0, 0, 0};
    }
    // extrema rows: the lane's accumulators, the window's first / last selected rows (acnt: its selected rows), are first / last asked for
    ExtremaAcc eacc[CPL];
    ExtremaRows erows{kExtNoRow, kExtNoRow};
    bool eends = false;
    if constexpr (EXT) eends = a.ext.first != nullptr || a.ext.last != nullptr;
    // histogram rows: the lane's columns and where the samples are counted
    HistCol hcol[CPL];
    HistCtx hctx{};
    if constexpr (HIST) {
#pragma unroll
        for (int k = 0; k < CPL; k++) hcol[k] = hist_col<W>(a, genk[k], col_ok[k]);
        hctx = hist_begin(a, smem);
    }
    // group-by rows: where the rows are added up (the block's rows wait in mrow)
    GroupByCtx gctx{};
    if constexpr (GBY) gctx = groupby_begin(a, smem);
    if constexpr (Q == kQueryFilter) {
#pragma unroll
        for (int k = 0; k < CPL; k++) fc[k] = filter_col<W>(a, genk[k], col_ok[k]);
        finv = filter_inv(a);
    }
    // linear filter rows: this lane's columns' weights, loaded once; lacc the block's eight partial sums over the lane's columns, lcarry what
    // the previous block's row 7 hands to this block's row 0, lfirst: no row of the chunk is done (fb, fcnt and fmb are the filter's)
    LinearCol lc[CPL];
    LinearCtx lctx{};
    uint32_t lacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t lself = 0, lcarry = 0, lnext = 0;
    uint32_t lfirst = 1;
    uint64_t lchunk = 0;
    if constexpr (LIN) {
#pragma unroll
        for (int k = 0; k < CPL; k++) lc[k] = linear_col(a, genk[k], col_ok[k]);
        lctx = linear_ctx(a);
    }
    // rolling rows: each column's running sum, the chunk's blocks done, the delta-run blocks behind this one in a row, is this block one of a run,
    // and the block's results -- [0] minima, [1] maxima, [2] sums -- of every column of the lane
    uint32_t rsum[ROLL ? CPL : 1];
    uint32_t rblk = 0, rrun = 0;
    bool rinrun = false;
    // (cumulative rows: [0] minima, [1] maxima, [2] and [3] the sums' low and high words)
    uint32_t rres[ROLL ? 3 : CUM ? 4 : 1][(ROLL || CUM) ? CPL : 1][8];
    if constexpr (ROLL) {
#pragma unroll
        for (int k = 0; k < CPL; k++) rsum[k] = 0;
    }
    // FIR rows: the lane's column's taps in the workgroup's table, its bias, scale and offset (loaded once), and the format
    const uint32_t* firt = nullptr;
    uint32_t firb = 0, firmode = 0;
    float firsc = 1.0f, firof = 0.0f;
    if constexpr (FIR) {
        firt = (const uint32_t*)(smem + a.table.table_off + (size_t)(kThreads >> LOG2DP) * (size_t)roll_ring_bytes(a.win.rows, D, ESZ)) + colk[0];
        firmode = a.filter.mode;
        firb = fir_bias(a, (uint32_t)colk[0]);
        if (!(firmode & kDeriveI32Bit)) { firsc = float_scale(a, (uint32_t)colk[0]); firof = float_offset(a, (uint32_t)colk[0]); }
    }
    // cumulative rows: each column's running min / max / sum (set at each chunk start)
    CumState cums[CUM ? CPL : 1];
    // derive rows: the row in front of the block being decoded (clean), no row of the chunk is done, and the bytes of a derived block
    uint32_t dlast[1] = {0};
    uint32_t dfirst = 1;
    const uint32_t dblk_bytes = DER ? 8u * pK * OSZ : 0u;
    auto q_row = [&](int k, int i) {                       // pv[k] carries garbage above bit W: the queries select the element
        if constexpr (Q == kQueryFilter) {                 // with SDWA, the filter with the mask of its difference (plain C++)
            fcm |= filter_hit<W>(fc[k], pv[k]) << i;
        } else if constexpr (AGG || HIST || EXT || LIN || SEG || ROLL || CUM || DER || FIR) {  // the column's 8 rows wait for q_block: one test of the mask byte a column
            arow[i] = pv[k];
        } else if constexpr (MOM || GBY) {                 // every slot's rows wait for q_window: the reference / key column's may come last
            mrow[k][i] = pv[k];
        } else if constexpr (Q != 0) {
            if constexpr (W == 16) {
                asm("v_max_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                    : "=v"(qmax[k]) : "v"(qmax[k]), "v"(pv[k]));
                if constexpr (Q == kQueryWindow)
                    asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                        : "=v"(qmin[k]) : "v"(qmin[k]), "v"(pv[k]));
                asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                    : "=v"(qbs[k]) : "v"(qbs[k]), "v"(pv[k]));
            } else {
                asm("v_max_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
                    : "=v"(qmax[k]) : "v"(qmax[k]), "v"(pv[k]));
                if constexpr (Q == kQueryWindow)
                    asm("v_min_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
                        : "=v"(qmin[k]) : "v"(qmin[k]), "v"(pv[k]));
                asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
                    : "=v"(qbs[k]) : "v"(qbs[k]), "v"(pv[k]));
            }
        }
    };
    auto q_block = [&](int k) {
        if constexpr (Q == kQueryFilter) {                 // a lane column past the last one contributes the identity
            fl |= col_ok[k] ? (fcm ^ finv) & 0xffu : 0u;
            fcm = 0;
        } else if constexpr (AGG) {                        // a block whose mask byte is 0 only moves the predictor on
            if (sm != 0) {
                uint32_t bs = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) aggregate_row<W>(arow[i], aggregate_sel<W>(sm, i), qmin[k], qmax[k], bs);
                qsum[k] += bs;
            }
        } else if constexpr (SEG) {                        // a block with no start and no end takes all 8 rows or none: no row loop
            if (seg_loop) {
                segment_rows8<W>(a, sblk, sst, gbase, (uint32_t)D, (uint32_t)genk[k], col_ok[k], [&](int i) { return arow[i]; }, qmin[k], qmax[k], qsum[k]);
            } else if (sblk.members != 0) {
                uint32_t bs = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) aggregate_row<W>(arow[i], AggregateSel{MASK, 0u}, qmin[k], qmax[k], bs);
                qsum[k] += bs;
            }
        } else if constexpr (HIST) {                       // (a lane column past the last one counts nothing)
            if (sm != 0 && col_ok[k]) hist_rows8<W>(hctx, hcol[k], arow, sm);
        } else if constexpr (EXT) {                        // fb blocks = 8 fb rows lie in front of the block
            if (sm != 0) extrema_rows8<W>(eacc[k], [&](int i) { return arow[i]; }, sm, 8u * fb, erows.first == kExtNoRow, eends);
        } else if constexpr (LIN) {                        // (a lane column past the last one has weights 0; the chunk's first row leaves for the seam pass)
            if (lctx.lag && lfirst && col_ok[k]) linear_slot<W>(a, lchunk, (uint32_t)D).first[genk[k]] = (U)arow[0];
            linear_rows8<W>(lc[k], [&](int i) { return arow[i]; }, lctx.lag, lfirst, lacc, lself, lnext);
        } else if constexpr (ROLL) {                       // (a lane column past the last one has no ring and no results)
            if (col_ok[k])
                rolling_step8<W>(a, rolling_ring<W>(rollp, a, (uint32_t)genk[k]), rblk, [&](int i) { return arow[i]; }, rsum[ROLL ? k : 0],
                                 !FIRE && SPRINTZ_ROLL_RUN_SHORTCUT && rinrun && rolling_run_settled(a, rrun),
                                 [&](uint32_t op, int j, uint32_t v) { rres[op == kRollMin ? 0 : op == kRollMax ? 1 : 2][k][j] = v; });
        } else if constexpr (CUM) {                        // (a lane column past the last one has no results)
            if (col_ok[k])
                cumulative_step8<W>(a, [&](int i) { return arow[i]; }, cums[CUM ? k : 0], [&](uint32_t op, int j, uint64_t v) {
                    if (op == kCumSum) {
                        rres[CUM ? 2 : 0][k][j] = (uint32_t)v;
                        rres[CUM ? 3 : 0][k][j] = (uint32_t)(v >> 32);
                    } else {
                        rres[op == kCumMin ? 0 : CUM ? 1 : 0][k][j] = (uint32_t)v;
                    }
                });
        } else if constexpr (FIR) {                        // (a lane column past the last one has no ring and no results; the chunk's first T - 1 rows leave for the seam pass)
            if (col_ok[k])
                fir_step8<W>(a, rolling_ring<W>(rollp, a, (uint32_t)genk[k]), rblk, [&](int i) { return arow[i]; }, [&](uint32_t j) { return firt[j * (uint32_t)D]; }, firb,
                             (a.lin.tmp && 8u * rblk + 1u < fir_ntaps(a)) ? fir_slot<W>(a, lchunk).first + genk[k] : nullptr, (uint32_t)D, [&](int j, uint32_t y) {
                                 if (firmode & kDeriveI32Bit) {
                                     rres[0][0][j] = y;
                                 } else {
                                     const float z = derive_value(y, firsc, firof);
                                     rres[0][0][j] = (firmode & 3u) == kFloatF32 ? __float_as_uint(z) : (firmode & 3u) == kFloatF16 ? float_to_f16(z) : float_to_bf16(z);
                                 }
                             });
        } else if constexpr (DER) {                        // (the chunk's first row leaves for the seam pass; the block's values leave in der_out)
            if (a.lin.lag && dfirst && col_ok[k]) linear_slot<W>(a, lchunk, (uint32_t)D).first[genk[k]] = (U)arow[0];
        } else if constexpr (MOM || GBY) {
        } else if constexpr (Q != 0) { qsum[k] += qbs[k]; qbs[k] = 0; }
    };
    // after every block of 8 rows: the group's lanes combine, one lane stores the block's byte (fb < chunk_len / blk_elems <=
    // mask_stride: the capacity guard has passed), every lane keeps the count
    auto f_block = [&]() {
        if constexpr (Q == kQueryFilter) {
            const uint32_t m = (group_or<DP>(fl) ^ finv) & 0xffu;
            fl = 0;
            if (fmb && lane_d == 0) fmb[fb] = (uint8_t)m;
            fcnt += (uint32_t)__popc(m);
            fb++;
        }
        if constexpr (LIN) {
            const uint32_t m = linear_block(lctx, lacc, lfirst, lself, lcarry, lnext, [](uint32_t v) { return group_add<DP>(v); });
            if (fmb && lane_d == 0) fmb[fb] = (uint8_t)m;
            fcnt += (uint32_t)__popc(m);
            fb++;
        }
    };
    // the windowed query's own form of window_advance (decode_ops.h), kept local as its tail below is: through the shared walk the
    // delta kernels of Q = kQueryWindow came out with other schedules (tools/kernel_diff.py), and this mode keeps its code
    auto win_flush_all = [&]() {                           // window wi of this chunk leaves, every genuine column of the lane
#pragma unroll
        for (int k = 0; k < CPL; k++)
            if (col_ok[k]) win_flush<W>(a, (wbase + wi) * (uint64_t)D + (uint64_t)genk[k], qmin[k], qmax[k], qsum[k]);
        wi++;
        wleft = a.win.rows;
    };
    // aggregate and moments rows: `n` rows of window wi of this chunk are done (window_advance); a window that leaves takes the
    // entries of every genuine column of the lane along, and its count of selected rows
    auto window_rows_done = [&](uint32_t n) {
        window_advance<true>(a, n, wbase, wi, wleft, acnt, lane_d, [&](uint64_t w) {
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (!col_ok[k]) continue;
                if constexpr (MOM) moments_flush(a, w * (uint64_t)D + (uint64_t)genk[k], macc[k]);
                else if constexpr (EXT) extrema_flush<W>(a, w * (uint64_t)D + (uint64_t)genk[k], eacc[k]);
                else win_flush<W>(a, w * (uint64_t)D + (uint64_t)genk[k], qmin[k], qmax[k], qsum[k]);
            }
            if constexpr (EXT) extrema_rows_flush(a, w, erows, lane_d);
        });
    };
    auto q_window = [&]() {                                // after every block of 8 rows
        if constexpr (Q == kQueryWindow) {
            wleft -= 8;
            if (wleft == 0) win_flush_all();
        }
        if constexpr (AGG) {                               // the block's selected rows are counted, then as above
            acnt += (uint32_t)__popc(sm);
            fb++;
            window_rows_done(8u);
        }
        if constexpr (HIST) fb++;
        if constexpr (SEG) {                               // the ended segments' rows and starts leave, the group's state moves on (fb blocks = 8 fb rows in front)
            segment_block_done(a, sblk, sst, gbase, grow0, 8u * fb, lane_d);
            fb++;
        }
        if constexpr (EXT) {                               // the window's first / last selected rows move behind the columns, then as aggregate
            if (sm != 0) extrema_rows8_done(erows, sm, 8u * fb);
            acnt += (uint32_t)__popc(sm);
            fb++;
            window_rows_done(8u);
        }
        if constexpr (MOM) {
            // sm is the group's: every lane of it takes part in the exchange, a lane whose columns are past the last one too (its
            // own sums are never flushed)
            if (sm != 0) {
                uint32_t xr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                const bool cross = a.mom.cross != nullptr;
                if (cross) moments_ref_rows<W, CPL>(a.mom.ref, DP, [&](int k, int i) { return mrow[k][i]; }, xr);
#pragma unroll
                for (int k = 0; k < CPL; k++) moments_rows8<W>(macc[k], [&](int i) { return mrow[k][i]; }, xr, sm, cross);
            }
            acnt += (uint32_t)__popc(sm);
            fb++;
            window_rows_done(8u);
        }
        if constexpr (GBY) {
            // sm is the group's: every lane of it takes part in the exchange of the key column's rows
            if (sm != 0) {
                uint32_t xk[8];
                moments_ref_rows<W, CPL>(a.gby.key, DP, [&](int k, int i) { return mrow[k][i]; }, xk);
                groupby_rows8<W, CPL>(gctx, [&](int k, int i) { return mrow[k][i]; }, xk, sm, genk, col_ok, lane_d);
            }
            fb++;
        }
    };
    uint32_t ovo = 0;                                      // output cursor (byte offset from this wave's out_base)
    // gather: the chunk-relative row of the next block, and the row of the block each of this lane's 16-byte store pieces lies in
    // (a row is a whole number of pieces and a block starts a row, so that is the same for every block)
    uint32_t grow = 0;
    uint32_t prow[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; q++) prow[q] = (GATHER || SELECT) ? (lane16 + (uint32_t)q * ROW16) / row_stride : 0u;
    const uint32_t gspan = gp.hi - gp.lo;
    // select: where in its row each of this lane's store pieces starts; the chunk's mask bytes, its first output row, its first batch row,
    // the set bits of its blocks done so far (fb counts those blocks, as for the filter) and the mask byte of the block being decoded
    uint32_t pcol[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; q++) pcol[q] = SELECT ? lane16 + (uint32_t)q * ROW16 - prow[q] * row_stride : 0u;
    // float rows: the scale and the offset of every element of each of this lane's store pieces (a row is a whole number of pieces, so piece
    // q starts in the same column of its row in every block); a piece past the block's end (never stored) reads some row's columns too
    constexpr int FNE = 128 / W;                           // elements of a 16-byte piece
    float fsc[(FLT || PROJ) ? PIECES : 1][FNE], fof[(FLT || PROJ) ? PIECES : 1][FNE];
    if constexpr (FLT) {
#pragma unroll
        for (int q = 0; q < PIECES; q++) {
            const uint32_t c0 = ((lane16 + (uint32_t)q * ROW16) % row_stride) / ESZ;
#pragma unroll
            for (int j = 0; j < FNE; j++) {
                fsc[q][j] = float_scale(a, c0 + (uint32_t)j);
                fof[q][j] = float_offset(a, c0 + (uint32_t)j);
            }
        }
    }
    // (project rows: a block is a whole number of pieces and of rows, so piece q starts in the same slot in every block -- but a piece may run
    //  over a row's end into the next row's first slots: element j is slot (c0 + j) % K's, always inside the K entries)
    if constexpr (PROJ) {
        if (pflt) {
#pragma unroll
            for (int q = 0; q < PIECES; q++) {
                uint32_t c = ((lane16 + (uint32_t)q * ROW16) / ESZ) % pK;
#pragma unroll
                for (int j = 0; j < FNE; j++) {
                    fsc[q][j] = float_scale(a, c);
                    fof[q][j] = float_offset(a, c);
                    c = c + 1u == pK ? 0u : c + 1u;
                }
            }
        }
    }
    // a held or immediate piece leaves converted: output piece j of it 16 j bytes behind vo, or nowhere
    auto float_store = [&](const uint4& t, int q, uint32_t vo) {
        if constexpr (FLT || PROJ) {
            float_piece<W>(t, a.filter.mode, fsc[q], fof[q], [&](int j, const uint4& p) {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, p), orsrc, vo == kDropStore ? kDropStore : vo + 16u * (uint32_t)j, 0, kStoreAux);
            });
        }
    };
    const uint8_t* smb = nullptr;
    uint64_t sbase = 0, srow0 = 0;
    uint32_t srank = 0;
    // The mask bytes are read ahead of the blocks, 4 DP of them at a time: lane l of the group keeps dword l of the window that starts at
    // byte mwin0 (a multiple of 4) of the chunk's mask, and a block's byte comes out of its lane's dword with one cross-lane read -- no
    // load from memory sits between a block's header and its stores.  (A chunk's mask starts at any address, and its last dword may be
    // short: those bytes are read one by one.)
    uint32_t mwin = 0, mwin0 = 0x80000000u;
    auto sel_byte = [&](uint32_t b) -> uint32_t {
        if (b - mwin0 >= 4u * DP) {
            mwin0 = b & ~3u;
            const uint32_t o = mwin0 + 4u * (uint32_t)lane_d;
            mwin = 0;
            if (o + 4u <= a.rows.stride) {
                mwin = *(const u32_unaligned*)(smb + o);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++)
                    if (o + j < a.rows.stride) mwin |= (uint32_t)smb[o + j] << (8u * j);
            }
        }
        const uint32_t i = b - mwin0;
        const uint32_t w = (uint32_t)__shfl((int)mwin, (int)(i >> 2), DP);
        return (w >> (8u * (i & 3u))) & 0xffu;
    };
    // after every block of 8 rows: the selected rows' numbers leave, the chunk's rank moves on
    auto s_block = [&]() {
        if constexpr (SELECT) {
            if (sm) select_ids(a, sbase + srank, sm, srow0 + 8u * fb, lane_d, DP);
            srank += (uint32_t)__popc(sm);
            fb++;
        }
    };

    // segment rows, in front of a block's columns: the block under the rule, and whether any group of the wavefront (of its lanes that are
    // here) must walk its rows -- one branch a wave instead of both sides of a divergent one
    auto seg_begin = [&]() {
        if constexpr (SEG) {
            sblk = segment_block(a.win.rows, sm, sst.open);
            seg_loop = __any(segment_block_plain(sblk) ? 0 : 1) != 0;
        }
    };

    // ---- per-block workers ------------------------------------------------------
    // The staged 8 x D block is contiguous in the output.  Packed blocks are read
    // back from LDS into `held[slot]` and stored at the BOTTOM of the group step by
    // unconditional dwordx4 buffer stores (a slot that produced no packed block
    // re-stores the previous one: same lane, same address, same data; before the
    // first block the offset is out of range and the hardware drops the store).
    uint4 held[2][PIECES];
    uint32_t held_vo[2][PIECES];
#pragma unroll
    for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
        for (int q = 0; q < PIECES; q++) { held[s2][q] = make_uint4(0, 0, 0, 0); held_vo[s2][q] = kDropStore; }
    // after the 8 rows sit in `stage`; slot < 0: store right away (run blocks)
    // column-major: the packed 8 samples of each of this lane's columns
    uint32_t pk[CPL][4];
    uint4 cheld[2][CPL];
    uint32_t cheld_vo[2][CPL];
    uint32_t cbase[CPL];                                   // byte offset of this lane's columns in the descriptor
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        cbase[k] = CM ? (uint32_t)((uint64_t)genk[k] * a.col_stride * ESZ) : 0u;
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) { cheld[s2][k] = make_uint4(0, 0, 0, 0); cheld_vo[s2][k] = kDropStore; }
    }
    auto store_col = [&](const uint4& t, uint32_t vo) {
        if constexpr (W == 16) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), orsrc, vo, 0, kStoreAux);
        } else {
            typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t v2u;
            v2u h = {t.x, t.y};
            __builtin_amdgcn_raw_buffer_store_b64(h, orsrc, vo, 0, kStoreAux);
        }
    };
    // Column-major burst (one column per lane): a lone 16-byte store per lane per block costs
    // more than the whole decode (0.36 vs 0.15 ms on 8M x 32; every request is its own cache
    // line).  So four blocks (two group steps) of every column wait in LDS as
    // cst[column][slot], and on every second step a QUAD of lanes stores one column's 64
    // contiguous bytes -- whole 64-byte requests, as in the row-major path.
    constexpr bool CMB = CM && CPL == 1;
    constexpr uint32_t PB = W == 16 ? 16u : 8u;            // bytes of one block of one column
    uint8_t* const cst = stage;
    uint32_t* const cvo = (uint32_t*)(stage + 4u * DCAP * PB);   // row offset of staged block b, or kDropStore
    uint32_t stepno = 0;
    const uint32_t cs_bytes = CM ? (uint32_t)(a.col_stride * ESZ) : 0u;
    // slot permutation: column c keeps block b at slot (b + c/4) % 4, which spreads both the
    // per-column writes and the per-quad reads over the banks
    auto cst_at = [&](uint32_t col, uint32_t blk) { return cst + (col * 4u + ((blk + (col >> 2)) & 3u)) * PB; };
    if constexpr (CMB) {
        if (lane_d < 4) cvo[lane_d] = kDropStore;
        wave_lds_sync();
    }
    // `real` = false: the same four store instructions, all dropped (keeps the VMEM count of a step fixed)
    auto cm_flush = [&](bool real) {
        if constexpr (CMB) {
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t pid = (uint32_t)j * DP + (uint32_t)lane_d, col = pid >> 2, p = pid & 3u;
                uint4 t = make_uint4(0, 0, 0, 0);
                uint32_t vo = kDropStore;
                if (real && col < (uint32_t)D) {
                    const uint32_t rofs_b = cvo[p];
                    if constexpr (W == 16) t = *(const uint4*)cst_at(col, p);
                    else { const uint2 h = *(const uint2*)cst_at(col, p); t.x = h.x; t.y = h.y; }
                    vo = rofs_b == kDropStore ? kDropStore : col * cs_bytes + rofs_b;
                }
                store_col(t, vo);
            }
            if (real) {
                wave_lds_sync();
                if (lane_d < 4) cvo[lane_d] = kDropStore;
            }
            wave_lds_sync();
        }
    };
    auto pack_row = [&](int k, int i) {                    // pv[k] is row i of the block
        if constexpr (CM) {
            if constexpr (W == 16) {
                if ((i & 1) == 0) pk[k][i >> 1] = pv[k] & 0xffffu;
                else pk[k][i >> 1] |= pv[k] << 16;
            } else {
                if ((i & 3) == 0) pk[k][i >> 2] = pv[k] & 0xffu;
                else pk[k][i >> 2] |= (pv[k] & 0xffu) << (8 * (i & 3));
            }
        }
    };
    // rolling rows: the block's results leave.  A plane is staged as the plain decode stages a block -- row i of column c at stage + i * row_stride +
    // c * ESZ -- and read back as this lane's 16-byte pieces; `run`: the block was one of a run
    auto roll_plane = [&](int which, uint32_t shift) __attribute__((always_inline)) {
        wave_lds_sync();                                   // (the pieces of the plane before have been read)
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!col_ok[k]) continue;
#pragma unroll
            for (int i = 0; i < 8; i++) *(U*)(stage_k[k] + i * row_stride) = (U)(rres[(ROLL || CUM) ? which : 0][(ROLL || CUM) ? k : 0][i] >> shift);
        }
        wave_lds_sync();
    };
    auto roll_out = [&](bool run) __attribute__((always_inline)) {
        if constexpr (ROLL) {
            // a descriptor an output, based like orsrc (wave-uniform: hipcc hoists them out of the step); the sum's counts 4 bytes an element
            // (rfs: element bytes -> sum bytes, as a shift)
            constexpr uint32_t rfs = ESZ == 1 ? 2u : 1u;
            const uint32_t rspan = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(out_span < 0xfffffff0ull ? out_span : 0xfffffff0ull));
            const uint32_t rspan4 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((out_span << rfs) < 0xfffffff0ull ? (out_span << rfs) : 0xfffffff0ull));
            const __amdgpu_buffer_rsrc_t rrs_min = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.min + wave_uniform64(out_base)), 0, rspan, 0x00020000);
            const __amdgpu_buffer_rsrc_t rrs_max = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.max + wave_uniform64(out_base)), 0, rspan, 0x00020000);
            const __amdgpu_buffer_rsrc_t rrs_sum = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.sum + wave_uniform64(out_base << rfs)), 0, rspan4, 0x00020000);
#pragma unroll
            for (int op = 0; op < 2; op++) {
                if (!(a.win.ops & (op == 0 ? kRollMin : kRollMax))) continue;
                roll_plane(op, 0u);
#pragma unroll
                for (int q = 0; q < PIECES; q++) {
                    const uint32_t u = lane16 + q * ROW16;
                    const bool in = u < blk_bytes;
                    const uint4 t = *(const uint4*)(stage + (in ? u : 0u));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), op == 0 ? rrs_min : rrs_max, in ? ovo + u : kDropStore, 0, kStoreAux);
                }
            }
            if (a.win.ops & kRollSum) {
                constexpr int NP = 32 / W, NE = 128 / W;   // planes of a sum, elements of a piece
                uint4 pl[NP][PIECES];
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    roll_plane(2, (uint32_t)(W * p));
#pragma unroll
                    for (int q = 0; q < PIECES; q++) {
                        const uint32_t u = lane16 + q * ROW16;
                        pl[p][q] = *(const uint4*)(stage + (u < blk_bytes ? u : 0u));
                    }
                }
#pragma unroll
                for (int q = 0; q < PIECES; q++) {
                    const uint32_t u = lane16 + q * ROW16;
                    const bool in = u < blk_bytes;
                    uint32_t z[NE];
#pragma unroll
                    for (int e = 0; e < NE; e++) {
                        z[e] = 0;
#pragma unroll
                        for (int p = 0; p < NP; p++) {
                            const uint32_t w4[4] = {pl[p][q].x, pl[p][q].y, pl[p][q].z, pl[p][q].w};
                            const uint32_t part = W == 16 ? (w4[e >> 1] >> (16 * (e & 1))) & 0xffffu : (w4[e >> 2] >> (8 * (e & 3))) & 0xffu;
                            z[e] |= part << (W * p);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NE / 4; j++) {
                        const uint4 t = make_uint4(z[4 * j], z[4 * j + 1], z[4 * j + 2], z[4 * j + 3]);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), rrs_sum, in ? ((ovo + u) << rfs) + 16u * (uint32_t)j : kDropStore, 0, kStoreAux);
                    }
                }
            }
            ovo += blk_bytes;
            rblk++;
            rrun = (!FIRE && run) ? rrun + 1u : 0u;
        }
    };
    // cumulative rows: the block's results leave through the plain decode's staging, as rolling rows' do.  The sums -- OB bytes each, NP = OB / ESZ
    // times the block's bytes -- are staged AS SUMS, in their output order, 8 / NP rows of the block at a pass: a pass fills exactly the block's
    // staging (8 / NP rows x D x OB = 8 D ESZ bytes), and its 16-byte pieces lie in the output as they lie in LDS, so a store instruction writes one
    // contiguous stretch.  (Joined from element-type planes instead, a lane's NP output pieces were 16 bytes of every 16 NP: the int64 sum's
    // stores took 6.4 ms on the headline batch -- profiles/cumulative_rows.txt.)
    auto cum_sum_out = [&](auto ob) __attribute__((always_inline)) {
        if constexpr (CUM) {
            constexpr int OB = decltype(ob)::value;
            constexpr int NP = OB / ESZ, RPP = 8 / NP;     // passes a block, rows a pass
            constexpr uint32_t cfs = NP == 2 ? 1u : NP == 4 ? 2u : 3u;      // element bytes -> sum bytes, as a shift
            const uint32_t cspan = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((out_span << cfs) < 0xfffffff0ull ? (out_span << cfs) : 0xfffffff0ull));
            const __amdgpu_buffer_rsrc_t crs_sum = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.sum + wave_uniform64(out_base << cfs)), 0, cspan, 0x00020000);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                wave_lds_sync();                           // (the pieces of the pass before have been read)
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    if (!col_ok[k]) continue;
#pragma unroll
                    for (int r = 0; r < RPP; r++) {
                        uint8_t* const at = stage + (uint32_t)r * (uint32_t)D * OB + (uint32_t)genk[k] * OB;
                        if constexpr (OB == 8) *(uint2*)at = make_uint2(rres[CUM ? 2 : 0][k][p * RPP + r], rres[CUM ? 3 : 0][k][p * RPP + r]);
                        else *(uint32_t*)at = rres[CUM ? 2 : 0][k][p * RPP + r];
                    }
                }
                wave_lds_sync();
#pragma unroll
                for (int q = 0; q < PIECES; q++) {
                    const uint32_t u = lane16 + q * ROW16;
                    const bool in = u < blk_bytes;
                    const uint4 t = *(const uint4*)(stage + (in ? u : 0u));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), crs_sum, in ? (ovo << cfs) + (uint32_t)p * blk_bytes + u : kDropStore, 0, kStoreAux);
                }
            }
        }
    };
    auto cum_out = [&]() __attribute__((always_inline)) {
        if constexpr (CUM) {
            // a descriptor an output, based like orsrc (wave-uniform: hipcc hoists them out of the step)
            const uint32_t cspan = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(out_span < 0xfffffff0ull ? out_span : 0xfffffff0ull));
            const __amdgpu_buffer_rsrc_t crs_min = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.min + wave_uniform64(out_base)), 0, cspan, 0x00020000);
            const __amdgpu_buffer_rsrc_t crs_max = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.win.max + wave_uniform64(out_base)), 0, cspan, 0x00020000);
#pragma unroll
            for (int op = 0; op < 2; op++) {
                if (!(a.win.ops & (op == 0 ? kCumMin : kCumMax))) continue;
                roll_plane(op, 0u);
#pragma unroll
                for (int q = 0; q < PIECES; q++) {
                    const uint32_t u = lane16 + q * ROW16;
                    const bool in = u < blk_bytes;
                    const uint4 t = *(const uint4*)(stage + (in ? u : 0u));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), op == 0 ? crs_min : crs_max, in ? ovo + u : kDropStore, 0, kStoreAux);
                }
            }
            if (a.win.ops & kCumSum) {                     // (wave-uniform: sum_bytes is the call's)
                if (a.win.count == 8u) cum_sum_out(std::integral_constant<int, 8>{});
                else cum_sum_out(std::integral_constant<int, 4>{});
            }
            ovo += blk_bytes;                              // (nothing else is staged in this mode: the next plane's own barrier comes first)
        }
    };
    // derive rows: the block's 8 x K values leave (see DER above)
    auto der_out = [&]() __attribute__((always_inline)) {
        if constexpr (DER) {
            const uint2* const wt = (const uint2*)(smem + a.table.table_off);
            const uint32_t dmode = a.filter.mode;
            uint32_t x[8];
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = arow[i] & MASK;
            const uint32_t xp = dfirst ? x[0] : dlast[0];
            wave_lds_sync();                               // (the pieces of the block before have been read)
            for (uint32_t k = 0; k < pK; k++) {
                const uint2 wu = wt[k * (uint32_t)D + (uint32_t)colk[0]];
                const uint32_t w = col_ok[0] ? wu.x : 0u, u = col_ok[0] ? wu.y : 0u;      // (a stand-in lane contributes nothing)
                uint32_t p[8];
                p[0] = w * x[0] + u * xp;
#pragma unroll
                for (int i = 1; i < 8; i++) p[i] = w * x[i] + u * x[i - 1];
                const uint32_t b = derive_bias(a, k);
                const float sc = (dmode & kDeriveI32Bit) ? 1.0f : float_scale(a, k), of = (dmode & kDeriveI32Bit) ? 0.0f : float_offset(a, k);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t s = group_add<DP>(p[i]) + b;
                    if (lane_d == (i & (DP - 1))) {
                        uint8_t* const at = stage + ((uint32_t)i * pK + k) * OSZ;
                        if (dmode & kDeriveI32Bit) {
                            *(uint32_t*)at = s;
                        } else {
                            const float z = derive_value(s, sc, of);
                            if ((dmode & 3u) == kFloatF32) *(uint32_t*)at = __float_as_uint(z);
                            else *(uint16_t*)at = (uint16_t)((dmode & 3u) == kFloatF16 ? float_to_f16(z) : float_to_bf16(z));
                        }
                    }
                }
            }
            wave_lds_sync();
            for (uint32_t uo = lane16; uo < dblk_bytes; uo += ROW16) {
                const uint4 t = *(const uint4*)(stage + uo);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), orsrc, ovo + uo, 0, kStoreAux);
            }
            ovo += dblk_bytes;
            dlast[0] = x[7];
            dfirst = 0;
        }
    };
    // FIR rows: the block's 8 results a column leave (see FIR above): OB bytes each, NP = OB / ESZ times the block's bytes, 8 / NP rows of the block at a
    // pass -- a pass fills exactly the block's staging, and its 16-byte pieces lie in the output as they lie in LDS
    auto fir_store = [&](auto ob) __attribute__((always_inline)) {
        if constexpr (FIR) {
            constexpr int OB = decltype(ob)::value;
            constexpr int NP = OB / ESZ, RPP = 8 / NP;     // passes a block, rows a pass
            constexpr uint32_t cfs = NP == 1 ? 0u : NP == 2 ? 1u : 2u;      // element bytes -> output bytes, as a shift
            const uint32_t fspan = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((out_span << cfs) < 0xfffffff0ull ? (out_span << cfs) : 0xfffffff0ull));
            const __amdgpu_buffer_rsrc_t frs = __builtin_amdgcn_make_buffer_rsrc((void*)((uint8_t*)a.out + wave_uniform64(out_base << cfs)), 0, fspan, 0x00020000);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                wave_lds_sync();                           // (the pieces of the pass before have been read)
                if (col_ok[0]) {
#pragma unroll
                    for (int r = 0; r < RPP; r++) {
                        uint8_t* const at = stage + (uint32_t)r * (uint32_t)D * OB + (uint32_t)genk[0] * OB;
                        if constexpr (OB == 4) *(uint32_t*)at = rres[0][0][p * RPP + r];
                        else *(uint16_t*)at = (uint16_t)rres[0][0][p * RPP + r];
                    }
                }
                wave_lds_sync();
#pragma unroll
                for (int q = 0; q < PIECES; q++) {
                    const uint32_t u = lane16 + q * ROW16;
                    const bool in = u < blk_bytes;
                    const uint4 t = *(const uint4*)(stage + (in ? u : 0u));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), frs, in ? (ovo << cfs) + (uint32_t)p * blk_bytes + u : kDropStore, 0, kStoreAux);
                }
            }
        }
    };
    auto fir_out = [&]() __attribute__((always_inline)) {
        if constexpr (FIR) {
            if ((firmode & kDeriveI32Bit) || (firmode & 3u) == kFloatF32) fir_store(std::integral_constant<int, 4>{});      // (wave-uniform: the format is the call's)
            else fir_store(std::integral_constant<int, 2>{});
            ovo += blk_bytes;
            rblk++;
        }
    };
    auto stage_out = [&](int slot) {
        if constexpr (query_reduce_only(Q)) return;
        if constexpr (ROLL) { roll_out(slot < 0); return; }
        if constexpr (CMB) {                               // ovo counts ROW bytes here
            if (slot >= 0) {
                const uint32_t blk = (stepno & 1u) * 2u + (uint32_t)slot;
                if (col_ok[0]) {
                    if constexpr (W == 16) *(uint4*)cst_at((uint32_t)col0, blk) = make_uint4(pk[0][0], pk[0][1], pk[0][2], pk[0][3]);
                    else *(uint2*)cst_at((uint32_t)col0, blk) = make_uint2(pk[0][0], pk[0][1]);
                }
                if (lane_d == 0) cvo[blk] = ovo;
            } else {                                       // run blocks: straight from the registers
                const uint4 t = W == 16 ? make_uint4(pk[0][0], pk[0][1], pk[0][2], pk[0][3]) : make_uint4(pk[0][0], pk[0][1], 0, 0);
                store_col(t, col_ok[0] ? cbase[0] + ovo : kDropStore);
            }
            ovo += 8u * ESZ;
            return;
        }
        if constexpr (CM) {
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint4 t = W == 16 ? make_uint4(pk[k][0], pk[k][1], pk[k][2], pk[k][3]) : make_uint4(pk[k][0], pk[k][1], 0, 0);
                const uint32_t vo = col_ok[k] ? cbase[k] + ovo : kDropStore;
                if (slot >= 0) { cheld[slot][k] = t; cheld_vo[slot][k] = vo; }
                else store_col(t, vo);
            }
            ovo += 8u * ESZ;
            return;
        }
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < PIECES; q++) {
            const uint32_t u = lane16 + q * ROW16;
            bool in = u < blk_bytes;
            if constexpr (GATHER) in = in && grow + prow[q] - gp.lo < gspan;   // the piece's row is one the range wants
            uint32_t vo = ovo + u;
            if constexpr (SELECT) {                        // the piece's row is one the mask wants, and its place is inside `out` (compared in 64 bits)
                const uint64_t p = select_place(sbase + srank, sm, prow[q]);
                in = in && ((sm >> prow[q]) & 1u) && p < a.select.capacity;
                vo = (uint32_t)p * row_stride + pcol[q];   // (select.capacity rows fit 32-bit offsets: the launch checks)
            }
            if constexpr (FLT || PROJ) vo = ovo + (u << fshift);   // ovo counts output bytes; the piece's OSZ / ESZ output pieces follow each other
            const uint4 t = *(const uint4*)(stage + (in ? u : 0u));
            if constexpr (FLT) {
                if (slot >= 0) { held[slot][q] = t; held_vo[slot][q] = in ? vo : kDropStore; }
                else float_store(t, q, in ? vo : kDropStore);
            } else if constexpr (PROJ) {                   // held as it is; converted, or not, where it is stored
                if (slot >= 0) { held[slot][q] = t; held_vo[slot][q] = in ? vo : kDropStore; }
                else if (pflt) float_store(t, q, in ? vo : kDropStore);
                else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), orsrc, in ? vo : kDropStore, 0, kStoreAux);
            } else
            if (slot >= 0) {
                held[slot][q] = t;
#ifdef SPRINTZ_ABL_NO_GSTORE
                held_vo[slot][q] = kDropStore;             // ablation: every block store is dropped by the descriptor
#elif defined(SPRINTZ_ABL_STORE_INTERLEAVE)
                {   // ablation (wrong output on purpose): the 8 groups of a wave write ONE contiguous kilobyte per store instruction
                    const uint32_t g = (threadIdx.x & 63u) >> LOG2DP, gbase = g * a.chunk_len * ESZ;
                    held_vo[slot][q] = in ? ((ovo - gbase) >> 7) * 1024u + g * 128u + u : kDropStore;
                }
#elif defined(SPRINTZ_ABL_STORE_SLOT0_ONLY)
                held_vo[slot][q] = (in && slot == 0) ? ovo + u : kDropStore;   // ablation: slot 1's store is dropped
#elif defined(SPRINTZ_ABL_STORE_HALF_LANES)
                held_vo[slot][q] = (in && (lane_d & 1) == 0) ? ovo + u : kDropStore;   // ablation: every second lane's 16 bytes are dropped
#else
                held_vo[slot][q] = in ? vo : kDropStore;
#endif
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, t), orsrc, in ? vo : kDropStore, 0, kStoreAux);
            }
        }
        wave_lds_sync();
        ovo += (FLT || PROJ) ? blk_bytes << fshift : blk_bytes;
    };
    auto run_blocks = [&](uint32_t len) {                  // RUN slot: `len` blocks of zero error (:828-958)
        if constexpr (Q == kQueryFilter && !FIRE) {
            // a delta run repeats the previous row 8 len times: one test of that row, then len bytes of 0x00 or 0xFF -- up to
            // 32 767 of them -- spread over the group's lanes
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < CPL; k++) v |= col_ok[k] ? (filter_hit<W>(fc[k], pv[k]) ^ finv) & 1u : 0u;
            const uint32_t hit = (group_or<DP>(v) ^ finv) & 1u;
            if (fmb) {
                const uint8_t byte = hit ? 0xffu : 0u;
                for (uint32_t j = (uint32_t)lane_d; j < len; j += DP) fmb[fb + j] = byte;
            }
            fcnt += hit ? 8u * len : 0u;
            fb += len;
            return;
        }
        if constexpr (LIN && !FIRE && SPRINTZ_LIN_RUN_SHORTCUT) {
            // a delta run repeats the previous row 8 len times, and the row in front of the run equals it (at the chunk's start: the zero
            // row, its own predecessor): every row of the run has s = bias + sum (w + u) pv -- one evaluation, then len bytes of 0x00 or
            // 0xFF spread over the group's lanes.  What the run's last row hands on is sum u pv.
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            if (len == 0) return;                          // (a padding slot holds no row)
            uint32_t sw = 0, su = 0;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t x = pv[k] & MASK;
                sw += lc[k].w * x;
                su += lc[k].u * x;
                if (lctx.lag && lfirst && col_ok[k]) linear_slot<W>(a, lchunk, (uint32_t)D).first[genk[k]] = (U)x;
            }
            const uint32_t hit = linear_hit(lctx, group_add<DP>(sw + su));
            if (fmb) {
                const uint8_t byte = hit ? 0xffu : 0u;
                for (uint32_t j = (uint32_t)lane_d; j < len; j += DP) fmb[fb + j] = byte;
            }
            fcnt += hit ? 8u * len : 0u;
            fb += len;
            lcarry = su;
            lfirst = 0;
            return;
        }
        if constexpr (Q == kQueryWindow && !FIRE) {
            // a delta run repeats the previous row 8 len times (method.tex:150): per window it touches, min / max take the row
            // once and the sum takes it times the run's rows in that window -- O(windows), not O(rows)
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            uint32_t rows = len * 8u;
            while (rows > 0) {
                const uint32_t n = rows < wleft ? rows : wleft;
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    const uint32_t x = pv[k] & MASK;
                    qmin[k] = x < qmin[k] ? x : qmin[k];
                    qmax[k] = x > qmax[k] ? x : qmax[k];
                    qsum[k] += (uint64_t)x * n;
                }
                rows -= n;
                wleft -= n;
                if (wleft == 0) win_flush_all();
            }
            return;
        }
        if constexpr (AGG && !FIRE) {
            // a delta run repeats the previous row 8 len times: per window it touches, the selected rows among them are counted
            // (run_selected_rows), min / max take the row once if there is one, and the sum takes it times their number
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            uint32_t blocks = len;
            while (blocks > 0) {
                const uint32_t nb = blocks < (wleft >> 3) ? blocks : (wleft >> 3);
                const uint32_t c = run_selected_rows(smb, fb, nb, lane_d, DP);
                if (c != 0) {
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        const uint32_t x = pv[k] & MASK;
                        qmin[k] = x < qmin[k] ? x : qmin[k];
                        qmax[k] = x > qmax[k] ? x : qmax[k];
                        qsum[k] += (uint64_t)x * c;
                    }
                    acnt += c;
                }
                blocks -= nb;
                fb += nb;
                window_rows_done(8u * nb);
            }
            return;
        }
        if constexpr (EXT && !FIRE && SPRINTZ_EXT_RUN_SHORTCUT) {
            // a delta run repeats the previous row 8 len times: per window it touches, the selected rows among them are counted and the
            // first and the last of them found (run_selected_span); if there is one, min and max take the row once, at that first row, the
            // window's first row takes it if it had none, and its last row is the run's last -- O(windows), not O(rows)
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            uint32_t blocks = len;
            while (blocks > 0) {
                const uint32_t nb = blocks < (wleft >> 3) ? blocks : (wleft >> 3);
                uint32_t f, l;
                const uint32_t c = run_selected_span(smb, fb, nb, lane_d, DP, f, l);
                if (c != 0) {
                    const bool fresh = erows.first == kExtNoRow;
#pragma unroll
                    for (int k = 0; k < CPL; k++) extrema_value(eacc[k], pv[k] & MASK, f, fresh);
                    extrema_value_done(erows, f, l);
                    acnt += c;
                }
                blocks -= nb;
                fb += nb;
                window_rows_done(8u * nb);
            }
            return;
        }
        if constexpr (MOM && !FIRE) {
            // a delta run repeats the previous row 8 len times: per window it touches, c = the selected rows among them (run_selected_rows),
            // and each sum takes its term times c.  The reference column's value is one exchange a run.
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            const uint32_t xr = moments_ref_value<W, CPL>(a.mom.ref, DP, pv);
            uint32_t blocks = len;
            while (blocks > 0) {
                const uint32_t nb = blocks < (wleft >> 3) ? blocks : (wleft >> 3);
                const uint32_t c = run_selected_rows(smb, fb, nb, lane_d, DP);
                if (c != 0) {
#pragma unroll
                    for (int k = 0; k < CPL; k++) moments_value(macc[k], pv[k] & MASK, xr, c);
                    acnt += c;
                }
                blocks -= nb;
                fb += nb;
                window_rows_done(8u * nb);
            }
            return;
        }
        if constexpr (GBY && !FIRE) {
            // a delta run repeats the previous row 8 len times: its key, and so its bin, is one -- each column adds its value times the
            // run's selected rows (run_selected_rows), one lane adds their number.  The key column's value is one exchange a run.
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            const uint32_t c = run_selected_rows(smb, fb, len, lane_d, DP);
            groupby_value<W, CPL>(gctx, pv, moments_ref_value<W, CPL>(a.gby.key, DP, pv), c, genk, col_ok, lane_d);
            fb += len;
            return;
        }
        if constexpr (HIST && !FIRE) {
            // a delta run repeats the previous row 8 len times: each column's value takes ONE add of the run's selected rows (run_selected_rows)
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            out_left -= len * blk_elems;
            const uint32_t c = run_selected_rows(smb, fb, len, lane_d, DP);
#pragma unroll
            for (int k = 0; k < CPL; k++)
                if (col_ok[k]) hist_value<W>(hctx, hcol[k], pv[k], c);
            fb += len;
            return;
        }
        if constexpr (SEG && !FIRE && SPRINTZ_SEG_RUN_SHORTCUT) {
            // a delta run repeats the previous row 8 len times.  One pass over its mask bytes (segment_run_plain): if they hold no start and
            // no end the run is O(1) -- inside the open segment min / max take the row once and the sum takes it times the run's rows, outside
            // any nothing happens.  If not, the run is replayed block by block below, on the constant row.
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            if (len != 0 && segment_run_plain(a.win.rows, smb, fb, len, sst.open, lane_d, DP)) {
                out_left -= len * blk_elems;
                if (sst.open) {
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        const uint32_t x = pv[k] & MASK;
                        qmin[k] = x < qmin[k] ? x : qmin[k];
                        qmax[k] = x > qmax[k] ? x : qmax[k];
                        qsum[k] += (uint64_t)x * (8u * len);
                    }
                }
                fb += len;
                return;
            }
        }
        if constexpr (SELECT && !FIRE) {
            // a delta run repeats the previous row and changes no state: a run none of whose rows the mask wants is stepped over
            // (its mask bytes lie inside the chunk's: the run fits the chunk slot)
            if ((uint64_t)len * blk_elems > out_left) { corrupt = true; return; }
            uint32_t any = 0;
            for (uint32_t j = (uint32_t)lane_d; j < len; j += DP) any |= smb[fb + j];
            if (group_or<DP>(any) == 0) {
                out_left -= len * blk_elems;
                fb += len;
                return;
            }
        }
        if constexpr (GATHER && !FIRE) {
            // a delta run repeats the previous row: the blocks in front of row lo change no state and store nothing
            uint32_t skip = grow + 8u <= gp.lo ? (gp.lo - grow) >> 3 : 0u;
            skip = skip < len ? skip : len;
            if ((uint64_t)skip * blk_elems > out_left) { corrupt = true; return; }
            out_left -= skip * blk_elems;
            ovo += skip * blk_bytes;
            grow += skip * 8u;
            len -= skip;
        }
        for (; len > 0; len--) {
            if constexpr (GATHER) { if (grow >= gp.hi) break; }   // row hi - 1 has left: the rest of the run is not replayed
            if (out_left < blk_elems) { corrupt = true; break; }
            out_left -= blk_elems;
            if constexpr (ROLL) rinrun = true;
            if constexpr (SELECT) {
                sm = sel_byte(fb);
                if (!FIRE && sm == 0) { fb++; continue; }   // (a FIRE run is replayed for its state, and staged only where a bit is set)
            }
            if constexpr (MASKED && !SELECT) sm = (MASK_GIVEN || smb) ? sel_byte(fb) : 0xffu;   // (a FIRE run is replayed for its state, block by block, as the window mode does)
            seg_begin();
            auto run_step = [&](int k, int coef) {
                if constexpr (W == 16 && FIRE) {            // pd[k] holds X (delta in its high half), see packed_block
                    pd[k] = mad_i16_hi(pd[k], coef, 0);
                    pv[k] = add_hi16(pv[k], pd[k]);
                } else {
                    const int delta = FIRE ? __builtin_amdgcn_sbfe(mad24(pd[k], coef, 0), W, W) : 0;
                    pv[k] += (uint32_t)delta;
                    pd[k] = delta;
                }
            };
            auto run_col = [&](int k) {
                int coef = FIRE ? fire_coef<W, false>(ctr[k]) : 0;
                if constexpr (FIRE && W == 16) {
                    if (a.quirk) coef = fire_coef_ref_run16(ctr[k], genk[k]);      // the reference decoder's run replay, on request
                }
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    run_step(k, coef);
                    q_row(k, i);
                    pack_row(k, i);
#ifndef SPRINTZ_ABL_NO_STAGE
                    if constexpr (!query_reduce_only(Q) && !CM && !ROLL && !CUM && !DER && !FIR)
                        if (!SELECT || sm != 0) *(U*)(stage_k[k] + i * (PROJ ? prs : row_stride)) = (U)pv[k];
#endif
                }
                q_block(k);
            };
            if (MERGE8 && merge8) {
#pragma unroll
                for (int j = 0; j < NPAIR; j++) {
                    const int k = 2 * j;
                    const int coef0 = FIRE ? fire_coef<W, false>(ctr[k]) : 0, coef1 = FIRE ? fire_coef<W, false>(ctr[k + 1]) : 0;
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        run_step(k, coef0);
                        run_step(k + 1, coef1);
                        *(uint16_t*)(stage_k[k] + i * row_stride) = (uint16_t)__builtin_amdgcn_perm(pv[k + 1], pv[k], 0x0c0c0400u);
                    }
                }
                if constexpr (CPL & 1) run_col(CPL - 1);
            } else {
#pragma unroll
                for (int k = 0; k < CPL; k++) run_col(k);
            }
            q_window();
            f_block();
            if constexpr (GATHER) {                        // (a FIRE run in front of row lo is replayed for its state, not staged out)
                if (grow + 8u > gp.lo) stage_out(-1); else ovo += blk_bytes;
                grow += 8u;
            } else if constexpr (SELECT) {
                if (sm != 0) stage_out(-1);
                s_block();
            } else if constexpr (CUM) {                    // (called here, not through stage_out: hipcc did not inline that lambda into the 8-bit kernels, and its captures went to scratch)
                cum_out();
            } else if constexpr (DER) {                    // (called here too, for the same reason)
                der_out();
            } else if constexpr (FIR) {
                fir_out();
            } else {
                stage_out(-1);
            }
        }
    };
    // Field fetch fused with zigzag^-1.  With z = bits [sh, sh+nb) of the loaded dword,
    // err = (z >> 1) ^ -(z & 1) = bfe_u(w, sh+1, nb-1) ^ bfe_i(w, sh, 1): both halves come
    // straight from the dword (3 VALU per sample instead of bfe + 3); for an empty column
    // (nb == 0) both widths are 0 and the field reads as 0.  The XOR lands in the UPPER
    // half of the register (SDWA dst_sel:WORD_1), i.e. it yields E = err << 16 directly,
    // which is what the FIRE step and the sign test want (W == 16); for W == 8 one shift follows (FIRE) or none (delta).
    auto fetch_rows = [&](int (&e)[CPL][8], uint32_t at, const uint32_t (&off)[CPL], const uint32_t (&nb)[CPL], uint32_t row_bytes) {
        if constexpr (W == 8 && CPL >= 2) {
            // 8 bits: a lane's two adjacent columns are two adjacent fields of at most 8 bits, at most 7 + 16 bits from the byte
            // the first one starts in -- ONE 32-bit window per row serves both (an address, a mask and a v_alignbyte less per
            // second column and row).  (A stand-in column repeats the last genuine one: the same window.)
#pragma unroll
            for (int j = 0; j < NPAIR; j++) {
                const int k = 2 * j;
                uint32_t p = at + (off[k] >> 3);
                const uint32_t sha = off[k] & 7u, shb = off[k + 1] - (off[k] & ~7u);
                const uint32_t w1a = nb[k] != 0 ? 1u : 0u, wma = nb[k] - w1a;
                const uint32_t w1b = nb[k + 1] != 0 ? 1u : 0u, wmb = nb[k + 1] - w1b;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t w = lds_rd32(p);
                    const uint32_t ea = __builtin_amdgcn_ubfe(w, sha + 1u, wma) ^ (uint32_t)__builtin_amdgcn_sbfe((int)w, sha, w1a);
                    const uint32_t eb = __builtin_amdgcn_ubfe(w, shb + 1u, wmb) ^ (uint32_t)__builtin_amdgcn_sbfe((int)w, shb, w1b);
                    e[k][i] = FIRE ? (int)ea << 8 : (int)ea;
                    e[k + 1][i] = FIRE ? (int)eb << 8 : (int)eb;
                    p += row_bytes;
                }
            }
            if constexpr (CPL % 2 == 0) return;
        }
#pragma unroll
        for (int k = (W == 8 && CPL >= 2) ? 2 * NPAIR : 0; k < CPL; k++) {
            uint32_t p = at + (off[k] >> 3);
            const uint32_t sh = off[k] & 7u;
            const uint32_t w1 = nb[k] != 0 ? 1u : 0u;      // width of the sign bit field
            const uint32_t wm = nb[k] - w1;                // width of the magnitude field
#pragma unroll
            for (int i = 0; i < 8; i++) {
#ifdef SPRINTZ_ABL_NO_FETCH
                const uint32_t w = p * 2654435761u;        // ablation: no LDS read, the address arithmetic stays
#else
                const uint32_t w = lds_rd32(p);
#endif
                const uint32_t mag = __builtin_amdgcn_ubfe(w, sh + 1u, wm);
                const int sgn = __builtin_amdgcn_sbfe((int)w, sh, w1);
                if constexpr (W == 16) {
                    int x;
                    asm("v_xor_b32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0"
                        : "=v"(x) : "v"(mag), "v"(sgn));
                    e[k][i] = x;                           // err << 16
                } else if constexpr (FIRE) {
                    e[k][i] = (int)(mag ^ (uint32_t)sgn) << 8;            // err << 8 (mag ^ sgn is err, sign and all)
                } else {
                    e[k][i] = (int)(mag ^ (uint32_t)sgn);                 // the delta itself: nothing to scale it for
                }
                p += row_bytes;
            }
        }
    };
    // zigzag^-1 is done; e[][] holds E = err << W (sign-extended to 32 bits); 8-bit delta coding: err itself
    auto packed_block = [&](const int (&e)[CPL][8], int slot) {   // forecast recurrence (:993-1150)
        if (out_left < blk_elems) { corrupt = true; return; }
        out_left -= blk_elems;
        if constexpr (ROLL) rinrun = false;
        if constexpr (MASKED) sm = (MASK_GIVEN || smb) ? sel_byte(fb) : 0xffu;   // (block fb < chunk_len / blk_elems <= rows.stride: the guard has passed)
        seg_begin();
        auto col_step = [&](int k, int i, int coef, int& grad) {
            if constexpr (W == 16 && FIRE) {
                // X = prev_delta*coef + E; delta = hi16(X): pd[k] carries X, never the shifted delta
                if (i & 1) grad = mad_i16_hi(pd[k], sign_of(e[k][i]), grad);   // sign(E) == sign(err)
                pd[k] = mad_i16_hi(pd[k], coef, e[k][i]);
                pv[k] = add_hi16(pv[k], pd[k]);
            } else if constexpr (W == 16) {
                pv[k] = add_hi16(pv[k], e[k][i]);                               // delta = E >> 16
            } else {
                int delta;
                if constexpr (FIRE) {
                    if (i & 1) grad = mad24(sign_of(e[k][i]), pd[k], grad);
                    delta = __builtin_amdgcn_sbfe(mad24(pd[k], coef, e[k][i]), W, W);
                } else {
                    delta = e[k][i];
                }
                pv[k] += (uint32_t)delta;
                pd[k] = delta;
            }
        };
        auto one_col = [&](int k) {
            int grad = 0;
            const int coef = FIRE ? fire_coef<W, false>(ctr[k]) : 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                col_step(k, i, coef, grad);
                q_row(k, i);
                pack_row(k, i);
#ifndef SPRINTZ_ABL_NO_STAGE
                if constexpr (!query_reduce_only(Q) && !CM && !ROLL && !CUM && !DER && !FIR)
                    if (!SELECT || sm != 0) *(U*)(stage_k[k] + i * (PROJ ? prs : row_stride)) = (U)pv[k];   // (a block whose mask byte is 0 is not staged)
#else
                asm volatile("" :: "v"(pv[k]));
#endif
            }
            q_block(k);
            if constexpr (FIRE) ctr[k] = wrap_counter<W>(ctr[k] + __builtin_amdgcn_sbfe(grad, 2, W - 2));   // sext_W(grad) >> 2
        };
        if (MERGE8 && merge8) {                            // a lane's two adjacent 8-bit columns: one 16-bit staging write per row
#pragma unroll
            for (int j = 0; j < NPAIR; j++) {
                const int k = 2 * j;
                int grad0 = 0, grad1 = 0;
                const int coef0 = FIRE ? fire_coef<W, false>(ctr[k]) : 0, coef1 = FIRE ? fire_coef<W, false>(ctr[k + 1]) : 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    col_step(k, i, coef0, grad0);
                    col_step(k + 1, i, coef1, grad1);
                    *(uint16_t*)(stage_k[k] + i * row_stride) = (uint16_t)__builtin_amdgcn_perm(pv[k + 1], pv[k], 0x0c0c0400u);
                }
                if constexpr (FIRE) {
                    ctr[k] = wrap_counter<W>(ctr[k] + __builtin_amdgcn_sbfe(grad0, 2, W - 2));
                    ctr[k + 1] = wrap_counter<W>(ctr[k + 1] + __builtin_amdgcn_sbfe(grad1, 2, W - 2));
                }
            }
            if constexpr (CPL & 1) one_col(CPL - 1);
        } else {
#pragma unroll
            for (int k = 0; k < CPL; k++) one_col(k);
        }
        q_window();
        f_block();
        if constexpr (CUM) cum_out(); else if constexpr (DER) der_out(); else if constexpr (FIR) fir_out(); else stage_out(slot);
        s_block();
        if constexpr (GATHER) grow += 8u;
    };
    auto run_length = [&](uint32_t at, uint32_t& nbytes) -> uint32_t {   // varint in blocks (:829-833)
        const uint32_t b0 = lds_rd8(at);
        uint32_t len = b0 & 0x7fu;
        nbytes = 1;
        if (b0 & 0x80u) { len |= lds_rd8(at + 1) << 7; nbytes = 2; }
        return len;
    };

    bool need_prime = true;
    for (uint64_t chunk = c_first; chunk < c_end; chunk++) {
    // ---- chunk start: find the stream, read its 8-byte header (format.h:48-62)
    const uint64_t off_c = a.offsets[chunk];
    {
        const uint64_t off = off_c;
        const uint64_t gap = off - (gabs + rp);            // bytes between the cursor and the next stream
        if (need_prime || gap > 16 || rp > (1u << 30)) {
            prime(off);
        } else {                                           // alignment padding: just step over it
            rp += (uint32_t)gap;
            rofs += (uint32_t)gap;
            if (rofs >= RB) rofs -= RB;
            ahead -= (uint32_t)gap;
        }
        need_prime = false;
    }
    uint32_t groups_left, remaining;
    uint64_t stream_len;
    {
        const uint32_t w0 = lds_rd32(ring + rofs), w1 = lds_rd32(ring + rofs + 4);
        uint32_t hbytes = 8, nd_hdr = w1 >> 16;
        groups_left = w0;
        remaining = w1 & 0xffffu;
        if (a.norle) {                                     // {u32 len; u16 ndims} / u64 len with ndims in bytes 6..7 (decode_kernel.h)
            const uint32_t len = w0 <= a.chunk_len ? w0 : 0u;
            nd_hdr = w0 <= a.chunk_len ? (a.norle == 2 ? w1 >> 16 : w1 & 0xffffu) : 0xffffffffu;
            hbytes = a.norle == 2 ? 8u : 6u;
            groups_left = len < 128u ? 0u : len / (16u * (uint32_t)D);
            remaining = len - groups_left * 16u * (uint32_t)D;
        }
        rp += hbytes;
        rofs += hbytes;
        if (rofs >= RB) rofs -= RB;
        ahead -= hbytes;
#pragma unroll
        for (int k = 0; k < CPL; k++) { pv[k] = 0; pd[k] = 0; ctr[k] = 0; qmax[k] = 0; qsum[k] = 0; }
        if constexpr (Q == kQueryWindow || AGG) {          // windows are relative to the chunk
#pragma unroll
            for (int k = 0; k < CPL; k++) qmin[k] = MASK;
            wi = 0;
            wleft = a.win.rows;
            wbase = chunk * (uint64_t)a.win.count;
        }
        if constexpr (MOM) {
#pragma unroll
            for (int k = 0; k < CPL; k++) macc[k] = MomentAcc{0, 0, 0};
            wi = 0;
            wleft = a.win.rows;
            wbase = chunk * (uint64_t)a.win.count;
        }
        if constexpr (EXT) {
#pragma unroll
            for (int k = 0; k < CPL; k++) eacc[k] = extrema_identity();
            erows = ExtremaRows{kExtNoRow, kExtNoRow};
            wi = 0;
            wleft = a.win.rows;
            wbase = chunk * (uint64_t)a.win.count;
        }
        if constexpr (MASKED) {                            // the chunk's mask bytes (null: every row), its blocks done, its window's selected rows
            fb = 0; sm = 0; acnt = 0;
            mwin0 = 0x80000000u;                           // no window yet: the first block loads one
            smb = (MASK_GIVEN || a.rows.mask) ? a.rows.mask + chunk * (uint64_t)a.rows.stride : nullptr;
        }
        if constexpr (SEG) {                               // no segment is open, the accumulators hold the identities
#pragma unroll
            for (int k = 0; k < CPL; k++) qmin[k] = MASK;
            sst = SegState{0, 0, 0};
            sblk = SegBlock{0, 0, 0};
            seg_loop = false;
            gbase = a.select.bases[chunk];
            grow0 = chunk * (uint64_t)a.select.rpc;
        }
        if constexpr (Q == kQueryFilter) {
            fb = 0; fcnt = 0; fl = 0; fcm = 0;
            fmb = a.filter.mask ? a.filter.mask + chunk * (uint64_t)a.filter.mask_stride : nullptr;
        }
        if constexpr (LIN) {
            fb = 0; fcnt = 0;
            fmb = a.filter.mask ? a.filter.mask + chunk * (uint64_t)a.filter.mask_stride : nullptr;
#pragma unroll
            for (int i = 0; i < 8; i++) lacc[i] = 0;
            lself = 0; lcarry = 0; lnext = 0;
            lfirst = 1;
            lchunk = chunk;
        }
        if constexpr (HIST) hctx.g = hist_of_chunk(a, chunk);
        if constexpr (GBY) groupby_of_chunk(a, gctx, chunk);
        if constexpr (ROLL) {                              // the ring restarts cold with every chunk: no slot is read before this chunk wrote it
#pragma unroll
            for (int k = 0; k < CPL; k++) rsum[k] = 0;
            rblk = 0; rrun = 0; rinrun = false;
        }
        if constexpr (CUM) {                               // the running values enter the chunk as the scan left them
#pragma unroll
            for (int k = 0; k < CPL; k++) cums[CUM ? k : 0] = col_ok[k] ? cumulative_enter<W>(a, chunk, (uint32_t)D, (uint32_t)genk[k]) : CumState{MASK, 0u, 0ull};
        }
        if constexpr (FIR) {                               // the ring restarts cold with every chunk: no slot is read before this chunk wrote it
            rblk = 0;
            lchunk = chunk;
        }
        if constexpr (DER) {                               // the chunk's first row is its own predecessor inside the launch
            dfirst = 1;
            dlast[0] = 0;
            lchunk = chunk;
        }
        if constexpr (SELECT) {
            srank = 0;
            sbase = a.select.bases[chunk];
            srow0 = chunk * (uint64_t)a.select.rpc;
        }
        out_left = a.chunk_len;
        ovo = (PROJ || DER) ? (uint32_t)((chunk - wave_first) * (uint64_t)pslot_elems * OSZ)
          : FLT ? (uint32_t)((chunk - wave_first) * (uint64_t)a.chunk_len * OSZ)
          : CM ? (uint32_t)((chunk - wave_first) * (uint64_t)rows_per_chunk * ESZ)
          : GATHER ? (uint32_t)(uint64_t)(gp.obase * ESZ)  // where the chunk's row 0 would land: only rows [lo, hi) are stored, and those lie in `out`
                 : (uint32_t)((chunk - wave_first) * (uint64_t)a.chunk_len * ESZ);
        corrupt = (int)nd_hdr != D;
        // a damaged header must not make the loop spin: every group takes at least its
        // header and two slot bytes (none in the run-less codecs) out of the stream
        stream_len = a.offsets[chunk + 1] - off_c;
        if ((uint64_t)groups_left * (hdr_bytes + (a.norle ? 0u : 2u)) > stream_len || groups_left > a.chunk_len / blk_elems + 2u) corrupt = true;
        if (corrupt) groups_left = 0;
    }

    while (groups_left > 0 && !corrupt) {
        if constexpr (GATHER) { if (grow >= gp.hi) break; }   // the piece is complete: nothing behind row hi - 1 is parsed
        groups_left--;
        // ---- request the units that fit now; they are parked at the bottom of this step
        {
            const uint32_t room = RB - ahead;              // ring bytes the parser no longer needs
            npend = 0;
#pragma unroll
            for (uint32_t k = 0; k < NPEND; k++) {
                const bool wanted = room >= (k + 1) * UNIT;
                request(pend[k], wanted);
                npend += wanted ? 1u : 0u;
            }
            ahead += npend * UNIT;
        }

        // ---- group header: 2*D fields of HB bits (sprintz_xff_rle.cpp:713-735); both slots'
        // nbits ride in one register (slot 0 in bits 0..15, slot 1 in 16..31)
        const uint32_t r = ring + rofs;                    // LDS address of the parse cursor
        uint32_t nb_both[CPL], lane_both = 0;
        uint32_t hw0 = 0, hw1 = 0;                         // (two columns of a lane: their header fields sit in one window per slot)
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            const uint32_t hbit0 = (uint32_t)colk[k] * HB, hbit1 = (uint32_t)(D + colk[k]) * HB;
            uint32_t s0 = hbit0 & 7u, s1 = hbit1 & 7u;
            if (k & 1) {                                   // the odd column reads its pair's window
                const uint32_t b0 = (uint32_t)colk[k - 1] * HB, b1 = (uint32_t)(D + colk[k - 1]) * HB;
                s0 = hbit0 - (b0 & ~7u);
                s1 = hbit1 - (b1 & ~7u);
            } else {
                hw0 = lds_rd32(r + (hbit0 >> 3));
                hw1 = lds_rd32(r + (hbit1 >> 3));
            }
            uint32_t f0 = __builtin_amdgcn_ubfe(hw0, s0, HB);
            uint32_t f1 = __builtin_amdgcn_ubfe(hw1, s1, HB);
            f0 += (f0 == (uint32_t)(W - 1));               // W-1 means W (:747-749)
            f1 += (f1 == (uint32_t)(W - 1));
            nb_both[k] = f0 | (f1 << 16);
            lane_both += col_ok[k] ? nb_both[k] : 0u;
        }
        uint32_t tot_both;
        uint32_t excl_both, excl_single = 0;
        if constexpr (SPLIT) {                             // columns 0 .. 63 are the pairs, lane by lane; the singles follow them
            uint32_t tot_pairs, tot_singles;
            excl_both = group_scan<DP>(nb_both[0] + nb_both[1], lane_d, tot_pairs);
            excl_single = tot_pairs + group_scan<DP>(col_ok[2] ? nb_both[2] : 0u, lane_d, tot_singles);
            tot_both = tot_pairs + tot_singles;
        } else {
            excl_both = group_scan<DP>(lane_both, lane_d, tot_both);
        }
        const uint32_t tot0 = tot_both & 0xffffu, tot1 = tot_both >> 16;
        uint32_t off0[CPL], off1[CPL], nb0[CPL], nb1[CPL];
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            uint32_t o_both = col_ok[k] ? (SPLIT && k == 2 ? excl_single : excl_both) : tot_both - nb_both[k];   // (a stand-in: where column D-1 starts)
            if constexpr (MERGE8 && !EXACT && !SPLIT) {    // (a stand-in for column D-2 -- the first of the last pair -- starts one field earlier)
                if ((k & 1) == 0 && !col_ok[k] && colk[k] != colk[k + 1]) o_both -= nb_both[k + 1];
            }
            off0[k] = o_both & 0xffffu;
            off1[k] = o_both >> 16;
            nb0[k] = nb_both[k] & 0xffffu;
            nb1[k] = nb_both[k] >> 16;
            excl_both += nb_both[k];
        }

        // ---- lay out both slots, then fetch both before computing either
        const uint32_t at0 = r + hdr_bytes;
        uint32_t len0 = 0, len1 = 0, bytes0, bytes1;
        const uint32_t rb0 = (tot0 + 7u) >> 3, rb1 = (tot1 + 7u) >> 3;
        // (run-less codecs: an all-zero block has no payload at all and stands for itself)
        if (tot0 == 0) { if (a.norle) { len0 = 1; bytes0 = 0; } else len0 = run_length(at0, bytes0); } else bytes0 = rb0 * 8u;
        const uint32_t at1 = at0 + bytes0;
        if (tot1 == 0) { if (a.norle) { len1 = 1; bytes1 = 0; } else len1 = run_length(at1, bytes1); } else bytes1 = rb1 * 8u;
        const uint32_t used = hdr_bytes + bytes0 + bytes1;
        int z0[CPL][8], z1[CPL][8];
        if (tot0 != 0) fetch_rows(z0, at0, off0, nb0, rb0);
        if (tot1 != 0) fetch_rows(z1, at1, off1, nb1, rb1);

        if (tot0 == 0) run_blocks(len0); else packed_block(z0, 0);
        if (!corrupt && !(GATHER && grow >= gp.hi)) { if (tot1 == 0) run_blocks(len1); else packed_block(z1, 1); }

        rp += used;
        rofs += used;
        if (rofs >= RB) rofs -= RB;
        ahead -= used;

        // ---- bottom of the step.  VMEM order inside one step is: the stream loads (top),
        // [rare: run-block stores], the block stores (here).  gfx950 has ONE in-order
        // counter for loads and stores, so parking the loads must not wait for the stores
        // just issued: with every VMEM op of the common path unconditional, hipcc emits
        // s_waitcnt vmcnt(<number of stores>) here instead of vmcnt(0).
        if constexpr (!query_reduce_only(Q) && CMB) {
            cm_flush((stepno & 1u) != 0);
            stepno++;
        } else if constexpr (!query_reduce_only(Q) && CM) {
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                for (int k = 0; k < CPL; k++) store_col(cheld[s2][k], cheld_vo[s2][k]);
        } else if constexpr (FLT) {                        // the held pieces are converted here, where they are stored
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                for (int q = 0; q < PIECES; q++) float_store(held[s2][q], q, held_vo[s2][q]);
        } else if constexpr (PROJ) {                       // one wave-uniform switch a step: the held pieces leave converted, or as they are
            if (pflt) {
#pragma unroll
                for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                    for (int q = 0; q < PIECES; q++) float_store(held[s2][q], q, held_vo[s2][q]);
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                    for (int q = 0; q < PIECES; q++)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, held[s2][q]), orsrc, held_vo[s2][q], 0, kStoreAux);
            }
        } else if constexpr (!query_reduce_only(Q) && !ROLL && !CUM && !DER && !FIR) {
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                for (int q = 0; q < PIECES; q++)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, held[s2][q]), orsrc, held_vo[s2][q], 0, kStoreAux);
        }
#pragma unroll
        for (uint32_t k = 0; k < NPEND; k++)
            if (k < npend) commit(pend[k]);
        wave_lds_sync();
    }

    if constexpr (CMB) {                                   // an odd number of steps leaves one step's blocks staged
        if (stepno & 1u) cm_flush(true);
        stepno = 0;
    }
    // ---- verbatim tail (:1171), straight from HBM
    const uint32_t out_elems = a.chunk_len - out_left;
    if constexpr (GATHER) {
        // (Two ways out of the kernel here, where there were five: with the earlier returns hipcc no longer proved the stream loads'
        //  descriptor wave-uniform and wrapped each ring load in a v_readfirstlane loop -- 40 - 53 v_readfirstlane a kernel against
        //  4 - 5 now, the gather 6 - 10 % slower.  Nothing in the source states that uniformity: count them after an edit here.)
        if (grow >= gp.hi && !corrupt) return;             // delivered in full: the range's entry keeps gather.rows
        gather_tail<W>(a, gp, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, lane_d, DP, corrupt || remaining > out_left,
                       gabs + rp + (uint64_t)remaining * ESZ > a.offsets[chunk + 1]);
        return;
    }
    if (!corrupt && remaining > out_left) corrupt = true;
    // the groups and the tail the header announces must end inside the stream: a truncated stream is damaged, whatever the
    // bytes behind it (the next stream's, or padding) decoded to
    if (!corrupt && gabs + rp + (uint64_t)remaining * ESZ > off_c + stream_len) corrupt = true;
    if constexpr (Q == kQueryFilter) {
        if (!corrupt) filter_tail<W, CPL>(a, chunk, a.comp + gabs + rp, remaining, (uint32_t)D, fb, lane_d, DP, fc, genk, col_ok, fcnt);
        if (lane_d == 0 && a.filter.counts) a.filter.counts[chunk] = fcnt;
    } else if constexpr (LIN) {
        // fb blocks lie in front of the tail; a damaged chunk has no row the seam pass may use
        if (!corrupt) linear_tail<W, CPL>(a, chunk, a.comp + gabs + rp, remaining, (uint32_t)D, fb, lane_d, DP, lc, genk, col_ok, lctx, lcarry, pv, fcnt);
        else linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
        if (lane_d == 0 && a.filter.counts) a.filter.counts[chunk] = fcnt;
    } else if constexpr (Q == kQueryWindow) {
        // window_tail and reduce_tail (decode_ops.h), kept local: through the shared helpers these kernels were scheduled differently
        // and measured 0.6 - 1.2 % slower on the headline and 80-column batches (profiles/decode_ops_ab.txt); this is their code
        if (!corrupt) {
            const uint8_t* t = a.comp + gabs + rp;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (!col_ok[k]) continue;
                uint32_t w = wi, left = wleft;
                for (uint32_t e = (uint32_t)genk[k]; e < remaining; e += (uint32_t)D) {
                    if (left == 0) {
                        win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)genk[k], qmin[k], qmax[k], qsum[k]);
                        w++;
                        left = a.win.rows;
                    }
                    left--;
                    const uint32_t x = tail_elem<W>(t, e);
                    qmin[k] = x < qmin[k] ? x : qmin[k];
                    qmax[k] = x > qmax[k] ? x : qmax[k];
                    qsum[k] += x;
                }
                for (; w < a.win.count; w++) win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)genk[k], qmin[k], qmax[k], qsum[k]);
            }
        }
    } else if constexpr (AGG) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt)
            aggregate_tail<W, CPL>(a, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, wbase, wi, wleft, qmin, qmax, qsum, acnt, lane_d,
                                   [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (SEG) {
        // fb blocks = 8 fb rows lie in front of the tail; the segment open behind the chunk's last row ends there
        if (!corrupt)
            segment_tail<W, CPL>(a, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, sst, gbase, grow0, qmin, qmax, qsum, lane_d,
                                 [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (MOM) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt)
            moments_tail<W, CPL>(a, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, wbase, wi, wleft, macc, acnt, lane_d,
                                 [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (EXT) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt)
            extrema_tail<W, CPL>(a, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, wbase, wi, wleft, eacc, erows, acnt, lane_d,
                                 [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (HIST) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt)
            hist_tail<W, CPL>(a, hctx, hcol, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (GBY) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt)
            groupby_tail<W, CPL>(a, gctx, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, genk, col_ok, lane_d, [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (Q == kQueryMaterialize || Q == kQueryReduceOnly) {
        if (!corrupt) {
            const uint8_t* t = a.comp + gabs + rp;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (!col_ok[k]) continue;
                for (uint32_t e = (uint32_t)genk[k]; e < remaining; e += (uint32_t)D) {
                    const uint32_t x = tail_elem<W>(t, e);
                    qmax[k] = x > qmax[k] ? x : qmax[k];
                    qsum[k] += x;
                }
                if (a.qres) a.qres[chunk * (uint64_t)D + (uint64_t)genk[k]] = a.qop == 1 ? (uint64_t)qmax[k] : qsum[k];
            }
        }
    }
    if constexpr (ROLL) {
        // the tail walks row by row at plain 64-bit addresses, then the chunk leaves its count and last rows for the seam pass (decode_ops.h)
        if (!corrupt) rolling_tail<W, CPL>(a, chunk, rollp, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, genk, col_ok, rsum);
        rolling_leave<W, CPL>(a, chunk, rollp, corrupt ? 0u : out_elems + remaining, (uint32_t)D, genk, col_ok, lane_d);
    } else if constexpr (FIR) {
        // the tail walks row by row at plain 64-bit addresses, taps from global memory, then the chunk leaves its count and last rows for the seam pass
        if (!corrupt) fir_tail<W, CPL>(a, chunk, rollp, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, genk, col_ok);
        fir_leave<W, CPL>(a, chunk, rollp, corrupt ? 0u : out_elems + remaining, (uint32_t)D, genk, col_ok, lane_d);
    } else if constexpr (CUM) {
        // the tail walks row by row at plain 64-bit addresses; in a call of one chunk the state behind it is the call's carry_out (decode_ops.h)
        if (!corrupt) cumulative_tail<W, CPL>(a, chunk, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, genk, col_ok, cums);
        cumulative_leave<W, CPL>(a, chunk, corrupt, (uint32_t)D, genk, col_ok, cums);
    } else if constexpr (DER) {
        // the tail's whole rows leave value by value, at plain 64-bit addresses, then the chunk's rows for the seam pass (decode_ops.h: derive_tail);
        // a damaged chunk has no row the seam pass may use
        if (!corrupt) derive_tail<W, CPL>(a, chunk, a.comp + gabs + rp, remaining, (uint32_t)D, out_elems / blk_elems, lane_d, DP, genk, col_ok, dlast);
        else linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
    } else if constexpr (PROJ) {
        // the tail's selected columns leave element by element, at plain 64-bit addresses (decode_ops.h: project_tail)
        if (!corrupt && remaining > 0) project_tail<W>(a, chunk, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, lane_d, DP);
    } else if constexpr (FLT) {
        // the tail converts element by element, at plain 64-bit addresses (decode_ops.h: float_tail)
        if (!corrupt && remaining > 0) float_tail<W>(a, chunk, a.comp + gabs + rp, out_elems, remaining, (uint32_t)D, lane_d, DP);
    } else if constexpr (SELECT) {
        // fb blocks = 8 fb rows lie in front of the tail
        if (!corrupt && remaining > 0)
            select_tail<W>(a, chunk, a.comp + gabs + rp, remaining, (uint32_t)D, 8u * fb, sbase, srank, lane_d, DP, [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if (!corrupt && remaining > 0 && !query_reduce_only(Q) && CM) {
        const uint8_t* t = a.comp + gabs + rp;
        U* const c0 = (U*)((uint8_t*)a.out + out_base + ovo);          // column 0 at the tail's first row
        for (uint32_t e = (uint32_t)lane_d; e < remaining; e += DP) {
            // tail_elem, spelled out: called here, the 16-bit column-major kernels of the plain decode come out with two address
            // additions in the other order (tools/kernel_diff.py), and the plain decode keeps its code
            const uint32_t x = ESZ == 1 ? (uint32_t)t[e] : (uint32_t)*(const u16_unaligned*)(t + 2 * e);
            c0[(uint64_t)(e % (uint32_t)D) * a.col_stride + e / (uint32_t)D] = (U)x;
        }
    } else if (!corrupt && remaining > 0 && !query_reduce_only(Q)) {
        const uint8_t* t = a.comp + gabs + rp;
        uint8_t* d = (uint8_t*)a.out + out_base + ovo;
        copy_verbatim(t, d, remaining * ESZ, (uint32_t)lane_d, (uint32_t)DP);
    }
    if (corrupt || remaining > 0) need_prime = true;       // cursor no longer at the next stream
    if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
    }   // chunk loop
    if constexpr (HIST) hist_end(a, hctx);
    if constexpr (GBY) groupby_end(a, gctx);
}

}  // namespace sprintz
