// decode_kernel.h -- batched Sprintz decoder for gfx950, generic lane mapping.
//
// Replaces (bit-exact on every stream the reference encoder emits):
//   decompress_rowmajor_xff_rle<>           sprintz_xff_rle.cpp:569-1179
//   decompress_rowmajor_delta_rle<>         sprintz_delta_rle.cpp:418-772
//   decompress_rowmajor_{delta,xff}_rle_lowdim<>  sprintz_delta_lowdim.cpp:398-794,
//                                                 sprintz_xff_lowdim.cpp:414-1119
// The 16-bit FIRE run replay implements the inverse of the reference ENCODER
// (coefficient << 12); the reference decoder's run path uses << 4
// (sprintz_xff_rle.cpp:894-901) and does not invert its own encoder there --
// see DESIGN.md "Reference decoder quirk".
#pragma once

#include "decode_ops.h"

namespace sprintz {

template <int W, bool FIRE, bool LOWDIM, int CPL, int Q = 0>
__global__ void __launch_bounds__(kThreads) decode_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    constexpr int HB = Elem<W>::HB;
    constexpr uint32_t MASK = Elem<W>::MASK;
    constexpr int ESZ = W / 8;
    // HIST (sprintz_mi355x_histogram_rows): the workgroup's lanes meet at two barriers -- behind the zeroing of its table and in front of
    // the table's merge (decode_ops.h: table_begin, table_end) -- so in this mode no lane leaves early: a group past the last chunk
    // (hlive false) and a chunk whose header is refused (hbad) walk on as empty streams.
    constexpr bool HIST = Q == kQueryHistogram;
    // GBY (sprintz_mi355x_groupby_rows): the same two barriers around its table, so the same rule -- TAB is
    // either mode.  The block's rows of every column wait behind the column loop for the key column's, as the moments' do.
    constexpr bool GBY = Q == kQueryGroupBy;
    constexpr bool TAB = HIST || GBY;
    constexpr bool MOM = Q == kQueryMoments;
    // EXT (sprintz_mi355x_extrema_rows): aggregate's windows, mask and count; a column keeps min / max with their rows and its first / last value
    constexpr bool EXT = Q == kQueryExtrema;
    // LIN (sprintz_mi355x_filter_linear): the filter's outputs for a predicate on a linear form over the row and the row in front of it; runs
    // are replayed block by block, as for the filter
    constexpr bool LIN = Q == kQueryLinear;
    // the modes that take the rows a mask names (decode_ops.h: RowMaskArgs), and those of them that count a window's selected rows
    // SEG (sprintz_mi355x_segment_rows): aggregate's accumulators over windows whose edges come from the mask, placed behind the chunk's base
    // (decode_ops.h: SegState, segment_rows8); runs are replayed block by block
    constexpr bool SEG = Q == kQuerySegment;
    // ROLL (sprintz_mi355x_rolling_rows): every sample leaves as its column's min / max / sum over the W rows that end at its row; the group's LDS is
    // the chunk's history ring (decode_ops.h: rolling_rows8), runs are replayed block by block
    constexpr bool ROLL = Q == kQueryRolling;
    // CUM (sprintz_mi355x_cumulative_rows): every sample leaves as its column's running min / max / sum from the batch's first row on; a lane keeps the
    // running values of its columns in registers, loaded at the chunk's start from the scan's table (decode_ops.h: cumulative_rows8)
    constexpr bool CUM = Q == kQueryCumulative;
    // DER (sprintz_mi355x_derive_rows): K linear forms of every row and the row in front of it leave as a dense [rows, K] output, a form at a time
    // (decode_ops.h: derive_rows8); nothing of the decoded block is stored or staged, runs are replayed block by block
    constexpr bool DER = Q == kQueryDerive;
    // FIR (sprintz_mi355x_fir_rows): every sample leaves as its column's tap filter over the T rows that end at its row, as int32 or converted; the group's
    // LDS is the chunk's history ring (decode_ops.h: fir_rows8), taps come from global memory, runs are replayed block by block
    constexpr bool FIR = Q == kQueryFir;
    constexpr bool MASKED = Q == kQuerySelect || Q == kQueryAggregate || HIST || MOM || GBY || EXT || SEG;
    constexpr bool COUNTED = Q == kQueryAggregate || MOM || EXT;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int DP = 1 << a.log2DP;
    const int D = a.D;
    const uint64_t gtid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane_d = (int)(threadIdx.x & (uint32_t)(DP - 1));
    GatherPiece gp{};
    uint64_t chunk_sel = gtid >> a.log2DP;
    if constexpr (Q == kQueryGather) {              // the group's piece instead of the group's chunk
        if (!gather_piece(a, chunk_sel, gp)) return;
        if (!gp.exists) {
            if (lane_d == 0) gather_fail(a, gp.range, kErrNoRow);
            return;
        }
        chunk_sel = gp.chunk;
    }
    bool hlive = true, hbad = false;
    HistCtx hctx{};
    GroupByCtx gctx{};
    if constexpr (TAB) {
        if constexpr (HIST) hctx = hist_begin(a, smem);
        else gctx = groupby_begin(a, smem);
        hlive = chunk_sel < a.nchunks;
        if (!hlive) chunk_sel = a.nchunks - 1;      // (any stream will do: none of it is read)
    }
    const uint64_t chunk = chunk_sel;
    if constexpr (!TAB) {
        if (chunk >= a.nchunks) return;             // whole groups leave together
    }

    const uint64_t off_c = a.offsets[chunk];
    const uint8_t* s = a.comp + off_c;
    // the stream ends where the next one starts (offsets has nchunks + 1 entries): a damaged header,
    // field or run length must never walk the input cursor past it (the output side is guarded below)
    const uint64_t slen64 = a.offsets[chunk + 1] - off_c;
    const uint32_t stream_len = slen64 < 0xffffffffull ? (uint32_t)slen64 : 0xffffffffu;
    U* const o = (U*)a.out + chunk * (uint64_t)a.chunk_len;
    const uint64_t cs = a.col_stride;
    U* const cm0 = (U*)a.out + (cs ? chunk * (uint64_t)(a.chunk_len / (uint32_t)a.D) : 0);   // column 0 at this chunk's first row
    uint8_t* const lds = smem + (size_t)(threadIdx.x >> a.log2DP) * a.lds_group_stride;

    // ---- 8-byte stream header (format.h:48-62)
    uint32_t groups_left, remaining, pos;
    if (TAB && !hlive) {
        groups_left = 0; remaining = 0; pos = 0;
    } else if (a.norle) {                                   // format.h:65-86; sprintz_delta.cpp:803-807, :832
        // norle == 2: compress8b_rowmajor_xff's 8-byte header, a u64 len whose bytes 6..7 hold ndims (sprintz_xff.cpp:58-63)
        const uint32_t len = load_u32_any(s);
        const uint32_t ndo = a.norle == 2 ? 6u : 4u;
        const uint32_t nd = load_u8(s + ndo) | (load_u8(s + ndo + 1) << 8);
        if ((int)nd != D || len > a.chunk_len) {
            if constexpr (Q == kQueryGather) { if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt); }
            else if (lane_d == 0 && a.rets) a.rets[chunk] = kErrCorrupt;
            if constexpr (LIN || DER) linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
            if constexpr (ROLL) rolling_mark<W>(a, chunk, lane_d);
            if constexpr (FIR) fir_mark<W>(a, chunk, lane_d);
            if constexpr (CUM) cumulative_mark(a, chunk, (uint32_t)D, lane_d, DP, W);
            if constexpr (TAB) hbad = true; else return;
        }
        groups_left = len < 128u ? 0u : len / (16u * (uint32_t)D);
        remaining = len - groups_left * 16u * (uint32_t)D;
        pos = a.norle == 2 ? 8u : 6u;
    } else if (!a.noheader) {
        const uint32_t w0 = load_u32_any(s), w1 = load_u32_any(s + 4);
        groups_left = w0;
        remaining = w1 & 0xffffu;
        pos = 8;
        if ((int)(w1 >> 16) != D) {
            if constexpr (Q == kQueryGather) { if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt); }
            else if (lane_d == 0 && a.rets) a.rets[chunk] = kErrCorrupt;
            if constexpr (LIN || DER) linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
            if constexpr (ROLL) rolling_mark<W>(a, chunk, lane_d);
            if constexpr (FIR) fir_mark<W>(a, chunk, lane_d);
            if constexpr (CUM) cumulative_mark(a, chunk, (uint32_t)D, lane_d, DP, W);
            if constexpr (TAB) hbad = true; else return;
        }
    } else {
        groups_left = a.nh_ngroups;
        remaining = a.nh_remaining;
        pos = 0;
    }

    const uint32_t hdr_bytes = (2u * (uint32_t)D * HB + 7u) >> 3;
    const uint32_t blk_elems = 8u * (uint32_t)D;
    // a damaged header must not make the loop spin: every group of a valid stream holds at
    // least one non-empty slot, except the one that closes the stream
    bool corrupt = groups_left > a.chunk_len / blk_elems + 2u || pos > stream_len;
    if (TAB && hbad) corrupt = true;
    if (corrupt) groups_left = 0;

    // per-column predictor state (all start at 0: sprintz_xff_rle.cpp:149-152)
    uint32_t pv[CPL];
    int pd[CPL], ctr[CPL];
    uint32_t nb0[CPL], nb1[CPL];     // nbits of the two slots of the current group
    uint32_t tot0 = 0, tot1 = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) { pv[k] = 0; pd[k] = 0; ctr[k] = 0; nb0[k] = 0; nb1[k] = 0; }

    uint32_t out_elems = 0;
    int slot = 2;
    uint32_t run_left = 0;
    // the row operations (decode_ops.h) take the lane's columns as a list: which they are, and which of them exist
    int colk[CPL];
    bool genk[CPL];
    uint32_t qmax[CPL];
    uint64_t qsum[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) { colk[k] = lane_d * CPL + k; genk[k] = colk[k] < D; qmax[k] = 0; qsum[k] = 0; }
    // windowed query: the window being accumulated and the rows it still takes
    // (set up in that mode alone: the other instantiations stay exactly as they were)
    uint32_t qmin[CPL];
    uint32_t wi = 0, wleft = 0;
    uint64_t wbase = 0;
    if constexpr (Q == kQueryWindow || Q == kQueryAggregate) {
#pragma unroll
        for (int k = 0; k < CPL; k++) qmin[k] = MASK;
        wleft = a.win.rows;
        wbase = chunk * (uint64_t)a.win.count;
    }
    // moments rows (MOM): the lane's accumulators; the windows are the windowed query's
    MomentAcc macc[CPL];
    if constexpr (MOM) {
#pragma unroll
        for (int k = 0; k < CPL; k++) macc[k] = MomentAcc{0, 0, 0};
        wleft = a.win.rows;
        wbase = chunk * (uint64_t)a.win.count;
    }
    // extrema rows (EXT): the lane's accumulators and the window's first / last selected rows; the windows are the windowed query's
    ExtremaAcc eacc[CPL];
    ExtremaRows erows{kExtNoRow, kExtNoRow};
    bool eends = false;
    if constexpr (EXT) {
#pragma unroll
        for (int k = 0; k < CPL; k++) eacc[k] = extrema_identity();
        eends = a.ext.first != nullptr || a.ext.last != nullptr;
        wleft = a.win.rows;
        wbase = chunk * (uint64_t)a.win.count;
    }
    // the masked modes: the chunk's mask bytes (null: every row), the mask byte of the block being decoded and the selected rows of the
    // window so far
    const uint8_t* smb = nullptr;
    uint32_t sm = 0xffu, acnt = 0;
    if constexpr (MASKED) {
        if (a.rows.mask) smb = a.rows.mask + chunk * (uint64_t)a.rows.stride;
    }
    // filter rows: each lane's columns' bounds, loaded once; the group ORs its lanes' block masks with wave shuffles (groups of up to
    // 64 lanes, both layouts), lane 0 stores the block's byte -- runs are replayed block by block here, as the decode does
    FilterCol fc[CPL];
    uint32_t finv = 0, fcnt = 0;
    uint8_t* fmb = nullptr;
    if constexpr (Q == kQueryFilter) {
#pragma unroll
        for (int k = 0; k < CPL; k++) fc[k] = filter_col<W>(a, colk[k], genk[k]);
        finv = filter_inv(a);
        if (a.filter.mask) fmb = a.filter.mask + chunk * (uint64_t)a.filter.mask_stride;
    }

    // linear filter rows: each lane's columns' weights, loaded once; the block's eight partial sums over the lane's columns and what the
    // previous block's row 7 hands to this block's row 0 (decode_ops.h: linear_rows8, linear_block); fcnt and fmb are the filter's
    LinearCol lc[CPL];
    LinearCtx lctx{};
    uint32_t lacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t lself = 0, lcarry = 0, lnext = 0;
    uint32_t lfirst = 1;
    if constexpr (LIN) {
#pragma unroll
        for (int k = 0; k < CPL; k++) lc[k] = linear_col(a, colk[k], genk[k]);
        lctx = linear_ctx(a);
        if (a.filter.mask) fmb = a.filter.mask + chunk * (uint64_t)a.filter.mask_stride;
    }

    // derive rows: each column's row in front of the block being decoded (the lag term's predecessor); no row of the chunk is done
    uint32_t dlast[DER ? CPL : 1];
    bool dfirst = true;
    if constexpr (DER) {
#pragma unroll
        for (int k = 0; k < CPL; k++) dlast[k] = 0;
    }

    // select rows: the chunk's first output row and the set bits of the blocks done so far
    uint64_t sbase = 0;
    uint32_t srank = 0;
    if constexpr (Q == kQuerySelect) sbase = a.select.bases[chunk];
    // segment rows: the group's walk over the chunk's segments (no segment is open, the accumulators hold the identities), the block being
    // decoded under the rule and the chunk's first batch row
    SegState sst{0, 0, 0};
    SegBlock sblk{0, 0, 0};
    uint64_t grow0 = 0;
    if constexpr (SEG) {
#pragma unroll
        for (int k = 0; k < CPL; k++) qmin[k] = MASK;
        sbase = a.select.bases[chunk];
        grow0 = chunk * (uint64_t)a.select.rpc;
    }
    // histogram rows: the lane's columns and the chunk's histogram
    HistCol hcol[CPL];
    if constexpr (HIST) {
#pragma unroll
        for (int k = 0; k < CPL; k++) hcol[k] = hist_col<W>(a, colk[k], genk[k]);
        hctx.g = hist_of_chunk(a, chunk);
    }
    // group-by rows: the chunk's table
    if constexpr (GBY) groupby_of_chunk(a, gctx, chunk);
    // float rows: each of the lane's columns' scale and offset, loaded once; the format and the sign bit (decode_ops.h: float_value)
    float fsc[CPL], fof[CPL];
    uint32_t ffmt = 0, fsb = 0;
    if constexpr (Q == kQueryFloat) {
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            fsc[k] = genk[k] ? float_scale(a, (uint32_t)colk[k]) : 1.0f;
            fof[k] = genk[k] ? float_offset(a, (uint32_t)colk[k]) : 0.0f;
        }
        ffmt = a.filter.mode & 3u;
        fsb = float_sign_bit<W>(a.filter.mode);
    }
    // project rows: each of the lane's columns' slot in the output row, K for "not selected" (any entry outside 0 .. K - 1), and the chunk's first row
    uint32_t pslot[CPL];
    uint32_t pK = 0;
    uint64_t prow0 = 0;
    if constexpr (Q == kQueryProject) {
        pK = project_k(a);
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            const uint32_t sl = genk[k] ? (uint32_t)project_slot(a, (uint32_t)colk[k]) : pK;
            pslot[k] = sl < pK ? sl : pK;
        }
        prow0 = chunk * (uint64_t)(a.chunk_len / (uint32_t)D);
    }
    // rolling rows: each column's running sum over its window; the chunk's ring is the group's LDS (a.table.table_off is 0 in this kernel's launch)
    uint32_t rsum[CPL];
    uint32_t rrun = 0;                               // the blocks of a delta run behind this one, in a row
    if constexpr (ROLL) {
#pragma unroll
        for (int k = 0; k < CPL; k++) rsum[k] = 0;
    }
    // cumulative rows: each column's running min / max / sum, entering the chunk as the scan left them
    CumState cst[CUM ? CPL : 1];
    if constexpr (CUM) {
#pragma unroll
        for (int k = 0; k < CPL; k++) cst[k] = genk[k] ? cumulative_enter<W>(a, chunk, (uint32_t)D, (uint32_t)colk[k]) : CumState{MASK, 0u, 0ull};
    }

    for (;;) {
        uint32_t z[8][CPL];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < CPL; k++) z[i][k] = 0;

        bool have = false;
        bool run_block = false;                  // this block is one of a RUN
        if (run_left > 0) {                      // inside a RUN: zero errors (sprintz_xff_rle.cpp:828-958)
            run_left--;
            have = true;
            run_block = true;
        } else {
            for (;;) {
                if (slot == 2) {
                    if (groups_left == 0) break;
                    if (hdr_bytes > stream_len - pos) { corrupt = true; break; }
                    groups_left--;
                    // group header: 2*D fields of HB bits, LSB-first (sprintz_xff_rle.cpp:713-735)
                    uint32_t s0 = 0, s1 = 0;
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        const int col = lane_d * CPL + k;
                        uint32_t f0 = 0, f1 = 0;
                        if (col < D) {
                            f0 = fetch_bits(s + pos, (uint32_t)col * HB, HB);
                            f1 = fetch_bits(s + pos, (uint32_t)(D + col) * HB, HB);
                        }
                        nb0[k] = f0 == (uint32_t)(W - 1) ? (uint32_t)W : f0;   // :747-749,763-765
                        nb1[k] = f1 == (uint32_t)(W - 1) ? (uint32_t)W : f1;
                        s0 += nb0[k];
                        s1 += nb1[k];
                    }
                    // both slot totals in one butterfly
                    const uint32_t both = group_sum(s0 | (s1 << 16), DP);
                    tot0 = both & 0xffffu;
                    tot1 = both >> 16;
                    pos += hdr_bytes;
                    slot = 0;
                }
                const uint32_t total = slot ? tot1 : tot0;
                if (total == 0 && a.norle) {     // a block of zeros: no payload at all
                    slot++;
                    have = true;
                    break;
                } else if (total == 0) {         // RUN slot: varint length in blocks (:829-833)
                    if (stream_len - pos < 2u) {     // room for the longest run length, or the stream is damaged
                        if (stream_len == pos || (load_u8(s + pos) & 0x80u)) { corrupt = true; break; }
                    }
                    const uint32_t b0 = load_u8(s + pos);
                    uint32_t len = b0 & 0x7fu;
                    if (b0 & 0x80u) { len |= load_u8(s + pos + 1) << 7; pos += 2; }
                    else pos += 1;
                    slot++;
                    if constexpr (HIST && !FIRE) {
                        // a delta run repeats the previous row 8 len times: each column's value takes ONE add of the run's selected rows
                        // (run_selected_rows: every lane of the group comes by)
                        if (len > 0) {
                            if ((uint64_t)out_elems + (uint64_t)len * blk_elems > a.chunk_len) { corrupt = true; break; }
                            const uint32_t c = run_selected_rows(smb, out_elems / blk_elems, len, lane_d, DP);
#pragma unroll
                            for (int k = 0; k < CPL; k++)
                                if (genk[k]) hist_value<W>(hctx, hcol[k], pv[k], c);
                            out_elems += len * blk_elems;
                        }
                        continue;
                    }
                    if constexpr (GBY && !FIRE) {
                        // a delta run repeats the previous row 8 len times: its key, and so its bin, is one -- each column adds its value
                        // times the run's selected rows, one lane their number; the key column's value is one exchange a run
                        if (len > 0) {
                            if ((uint64_t)out_elems + (uint64_t)len * blk_elems > a.chunk_len) { corrupt = true; break; }
                            const uint32_t c = run_selected_rows(smb, out_elems / blk_elems, len, lane_d, DP);
                            groupby_value<W, CPL>(gctx, pv, moments_ref_value<W, CPL>(a.gby.key, DP, pv), c, colk, genk, lane_d);
                            out_elems += len * blk_elems;
                        }
                        continue;
                    }
                    if (len > 0) { run_left = len - 1; have = true; run_block = true; break; }
                    // len == 0: padding slot, look at the next one
                } else {                         // packed block
                    uint32_t cur[CPL], lane_bits = 0;
#pragma unroll
                    for (int k = 0; k < CPL; k++) { cur[k] = slot ? nb1[k] : nb0[k]; lane_bits += cur[k]; }
                    uint32_t tot_unused;
                    uint32_t off = group_excl_scan(lane_bits, lane_d, DP, tot_unused);
                    if ((LOWDIM ? total : ((total + 7u) >> 3) << 3) > stream_len - pos) { corrupt = true; break; }
                    if constexpr (!LOWDIM) {
                        // row r: LSB-first bit stream of the D fields, padded to a byte (:961-990)
                        const uint32_t row_bits = ((total + 7u) >> 3) << 3;
#pragma unroll
                        for (int k = 0; k < CPL; k++) {
#pragma unroll
                            for (int i = 0; i < 8; i++)
                                z[i][k] = fetch_bits(s + pos, (uint32_t)i * row_bits + off, cur[k]);
                            off += cur[k];
                        }
                        pos += row_bits;         // 8 rows * row_bytes
                    } else {
                        // column-major: nbits[d] bytes per column (sprintz_delta_lowdim.cpp:561-603)
#pragma unroll
                        for (int k = 0; k < CPL; k++) {
#pragma unroll
                            for (int i = 0; i < 8; i++)
                                z[i][k] = fetch_bits(s + pos, off * 8u + (uint32_t)i * cur[k], cur[k]);
                            off += cur[k];
                        }
                        pos += total;
                    }
                    slot++;
                    have = true;
                    break;
                }
            }
        }
        if (!have || corrupt) break;
        if (out_elems + blk_elems > a.chunk_len) { corrupt = true; break; }   // never write outside the chunk slot

        // ---- zigzag^-1 + forecast recurrence, lane-local down each column (:993-1150)
        uint32_t v[8][CPL];
        uint32_t fl = 0;                         // filter: this lane's columns' rows, inverted domain
        // (block out_elems / blk_elems < chunk_len / blk_elems <= mask_stride: checked above; all 8 rows of a block exist)
        // (select and aggregate rows always have a mask: no test for them)
        if constexpr (MASKED) sm = (Q == kQuerySelect || Q == kQueryAggregate || SEG || smb) ? (uint32_t)smb[out_elems / blk_elems] : 0xffu;
        if constexpr (SEG) sblk = segment_block(a.win.rows, sm, sst.open);
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            int coef = FIRE ? fire_coef<W, LOWDIM>(ctr[k]) : 0;
            if constexpr (FIRE && W == 16 && !LOWDIM) {
                if (a.quirk && run_block) coef = fire_coef_ref_run16(ctr[k], lane_d * CPL + k);
            }
            int grad = 0;
            uint32_t pvk = pv[k];
            int pdk = pd[k];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int err = unzigzag(z[i][k]);
                const int pred = FIRE ? fire_predict<W, LOWDIM>(pdk, coef) : 0;
                const int delta = sext<W>(err + pred);
                if (FIRE && (i & 1)) grad += sign_times(err, pdk);
                pvk = (pvk + (uint32_t)delta) & MASK;
                pdk = delta;
                v[i][k] = (!FIRE && a.raw) ? z[i][k] : pvk;     // raw: the packed bits ARE the samples (sprintz_delta.cpp:143-146)
            }
            pv[k] = pvk;
            pd[k] = pdk;
            if (FIRE) ctr[k] = wrap_counter<W>(ctr[k] + (sext<W>(grad) >> 2));   // :1120-1128
            if constexpr (Q == kQueryFilter) {
                uint32_t cm = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) cm |= filter_hit<W>(fc[k], v[i][k]) << i;
                fl |= genk[k] ? (cm ^ finv) & 0xffu : 0u;
            } else if constexpr (Q == kQueryAggregate) {
                if (sm) {                        // (a block none of whose rows the mask names only moves the predictor on)
                    uint32_t bs = 0;
#pragma unroll
                    for (int i = 0; i < 8; i++) aggregate_row<W>(v[i][k], aggregate_sel<W>(sm, i), qmin[k], qmax[k], bs);
                    qsum[k] += bs;
                }
            } else if constexpr (SEG) {          // (a block with no start, no end and no member only moves the predictor on)
                if ((sblk.members | sblk.ends) != 0)
                    segment_rows8<W>(a, sblk, sst, sbase, (uint32_t)D, (uint32_t)colk[k], genk[k], [&](int i) { return v[i][k]; }, qmin[k], qmax[k], qsum[k]);
            } else if constexpr (HIST) {
                if (sm != 0 && genk[k]) {
                    uint32_t xs[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) xs[i] = v[i][k];
                    hist_rows8<W>(hctx, hcol[k], xs, sm);
                }
            } else if constexpr (EXT) {
                if (sm) extrema_rows8<W>(eacc[k], [&](int i) { return v[i][k]; }, sm, out_elems / (uint32_t)D, erows.first == kExtNoRow, eends);
            } else if constexpr (LIN) {          // (a lane column past the last one has weights 0; the chunk's first row leaves for the seam pass)
                if (lctx.lag && lfirst && genk[k]) linear_slot<W>(a, chunk, (uint32_t)D).first[colk[k]] = (U)v[0][k];
                linear_rows8<W>(lc[k], [&](int i) { return v[i][k]; }, lctx.lag, lfirst, lacc, lself, lnext);
            } else if constexpr (ROLL) {
                // (a delta run whose last W + 8 rows fill the ring is settled -- decode_ops.h; rrun is the group's, every column's alike)
                if (genk[k])
                    rolling_rows8<W>(a, rolling_ring<W>(lds + a.table.table_off, a, (uint32_t)colk[k]), out_elems / blk_elems, [&](int i) { return v[i][k]; }, rsum[k],
                                     chunk * (uint64_t)a.chunk_len + out_elems + (uint64_t)colk[k], (uint32_t)D,
                                     !FIRE && SPRINTZ_ROLL_RUN_SHORTCUT && run_block && rolling_run_settled(a, rrun));
            } else if constexpr (FIR) {          // (a.table.table_off is 0 in this kernel's launch)
                if (genk[k])
                    fir_rows8<W>(a, chunk, rolling_ring<W>(lds + a.table.table_off, a, (uint32_t)colk[k]), out_elems / blk_elems, [&](int i) { return v[i][k]; },
                                 chunk * (uint64_t)a.chunk_len + out_elems + (uint64_t)colk[k], (uint32_t)D, (uint32_t)colk[k]);
            } else if constexpr (CUM) {
                if (genk[k])
                    cumulative_rows8<W>(a, [&](int i) { return v[i][k]; }, cst[k], chunk * (uint64_t)a.chunk_len + out_elems + (uint64_t)colk[k], (uint32_t)D);
            } else if constexpr (MOM || GBY) {   // (the products / the adds wait for the reference / key column's rows: behind the column loop)
            } else if constexpr (Q != 0) {       // the query functor sees every decoded row (sprintz_xff_rle_query.hpp:346-596)
                uint32_t bs = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    qmax[k] = v[i][k] > qmax[k] ? v[i][k] : qmax[k];
                    if constexpr (Q == kQueryWindow) qmin[k] = v[i][k] < qmin[k] ? v[i][k] : qmin[k];
                    bs += v[i][k];
                }
                qsum[k] += bs;
            }
        }
        if constexpr (MOM) {
            // the reference column's 8 rows come from the lane that decoded them -- every lane of the group takes part, sm is the group's --
            // then each column's rows are multiplied and added
            if (sm != 0) {
                uint32_t xr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                const bool cross = a.mom.cross != nullptr;
                if (cross) moments_ref_rows<W, CPL>(a.mom.ref, DP, [&](int k, int i) { return v[i][k]; }, xr);
#pragma unroll
                for (int k = 0; k < CPL; k++) moments_rows8<W>(macc[k], [&](int i) { return v[i][k]; }, xr, sm, cross);
            }
        }
        if constexpr (GBY) {
            // the key column's 8 rows come from the lane that decoded them -- every lane of the group takes part, sm is the group's
            if (sm != 0) {
                uint32_t xk[8];
                moments_ref_rows<W, CPL>(a.gby.key, DP, [&](int k, int i) { return v[i][k]; }, xk);
                groupby_rows8<W, CPL>(gctx, [&](int k, int i) { return v[i][k]; }, xk, sm, colk, genk, lane_d);
            }
        }
        if constexpr (Q == kQueryWindow || COUNTED) {
            // the block's 8 rows lie in one window: it leaves when they complete it.  This is window_advance (decode_ops.h) written out:
            // called here, hipcc gave three of the aggregate kernels with 8 columns a lane scratch or a wave less (tools/kernel_regs.sh)
            if constexpr (COUNTED) acnt += (uint32_t)__popc(sm);
            if constexpr (EXT) {
                if (sm) extrema_rows8_done(erows, sm, out_elems / (uint32_t)D);
            }
            wleft -= 8;
            if (wleft == 0) {
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    const int col = lane_d * CPL + k;
                    if (col >= D) continue;
                    if constexpr (MOM) moments_flush(a, (wbase + wi) * (uint64_t)D + (uint64_t)col, macc[k]);
                    else if constexpr (EXT) extrema_flush<W>(a, (wbase + wi) * (uint64_t)D + (uint64_t)col, eacc[k]);
                    else win_flush<W>(a, (wbase + wi) * (uint64_t)D + (uint64_t)col, qmin[k], qmax[k], qsum[k]);
                }
                if constexpr (EXT) extrema_rows_flush(a, wbase + wi, erows, lane_d);
                if constexpr (COUNTED) window_count_flush(a, wbase + wi, acnt, lane_d);
                wi++;
                wleft = a.win.rows;
            }
        }

        if constexpr (ROLL) rrun = (!FIRE && run_block) ? rrun + 1u : 0u;

        if constexpr (DER) {
            // the chunk's first row leaves for the seam pass; then the block's 8 x K values, each at its place (out_elems + blk_elems <= chunk_len:
            // checked above, so the rows lie inside the chunk's R); 64-bit addresses, so this kernel takes every layout, every K and every alignment
            if (dfirst && a.lin.lag) {
#pragma unroll
                for (int k = 0; k < CPL; k++)
                    if (genk[k]) linear_slot<W>(a, chunk, (uint32_t)D).first[colk[k]] = (U)v[0][k];
            }
            derive_rows8<CPL>(a, chunk * (uint64_t)(a.chunk_len / (uint32_t)D) + out_elems / (uint32_t)D, (uint32_t)D, lane_d, DP, colk, genk, [&](int c, int i) { return v[i][c]; }, dfirst, dlast,
                              [&](uint32_t x) { return group_sum(x, DP); });
            dfirst = false;
        }

        if constexpr (SEG) segment_block_done(a, sblk, sst, sbase, grow0, out_elems / (uint32_t)D, lane_d);   // behind the block's columns

        if constexpr (Q == kQueryFilter) {       // block out_elems / blk_elems < chunk_len / blk_elems <= mask_stride (checked above)
            const uint32_t m = (group_or_any(fl, DP) ^ finv) & 0xffu;
            if (fmb && lane_d == 0) fmb[out_elems / blk_elems] = (uint8_t)m;
            fcnt += (uint32_t)__popc(m);
        }

        if constexpr (LIN) {                     // the same place as the filter's byte
            const uint32_t m = linear_block(lctx, lacc, lfirst, lself, lcarry, lnext, [&](uint32_t x) { return group_sum(x, DP); });
            if (fmb && lane_d == 0) fmb[out_elems / blk_elems] = (uint8_t)m;
            fcnt += (uint32_t)__popc(m);
        }

        // ---- store the 8 x D block (contiguous 8*D*ESZ bytes of the output)
        U* const ob = o + out_elems;
        if constexpr (query_reduce_only(Q) || ROLL || CUM || DER || FIR) {       // (FIR rows: as rolling rows; derive rows: the block's values left above; rolling rows: the block's results left from the column loop, the raw rows went to the ring; cumulative rows: likewise, no ring)
            (void)ob;
        } else if constexpr (Q == kQueryGather) {
            // rows [lo, hi) of the chunk alone, each at its place in the range; the parse stops after row hi - 1
            (void)ob;
            const uint32_t r0 = out_elems / (uint32_t)D;
            const int64_t eb = gp.obase + (int64_t)out_elems;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col < D) {
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        if (r0 + (uint32_t)i >= gp.lo && r0 + (uint32_t)i < gp.hi) ((U*)a.out)[eb + (int64_t)(i * D + col)] = (U)v[i][k];
                }
            }
            if (r0 + 8u >= gp.hi) return;            // delivered in full: the range's entry keeps gather.rows
        } else if constexpr (Q == kQuerySelect) {
            // the block's rows whose bits are set, each at its place behind the chunk's base (block out_elems / blk_elems <
            // chunk_len / blk_elems <= mask_stride: checked above); 64-bit addresses, a place >= capacity is dropped
            (void)ob;
            const uint32_t r0 = out_elems / (uint32_t)D;
            const uint32_t m = sm;
            const uint64_t first = sbase + srank;
            if (m) {
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    const int col = lane_d * CPL + k;
                    if (col < D) {
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const uint64_t p = select_place(first, m, (uint32_t)i);
                            if (((m >> i) & 1u) && p < a.select.capacity) ((U*)a.out)[p * (uint64_t)D + (uint64_t)col] = (U)v[i][k];
                        }
                    }
                }
                select_ids(a, first, m, chunk * (uint64_t)a.select.rpc + r0, lane_d, DP);
            }
            srank += (uint32_t)__popc(m);
        } else if constexpr (Q == kQueryFloat) {
            // every sample converted, at the plain decode's place (out_elems + blk_elems <= chunk_len: checked above); 64-bit addresses, so
            // this kernel takes every layout, every row length and every alignment of the output the element size allows
            (void)ob;
            const uint64_t eb = chunk * (uint64_t)a.chunk_len + out_elems;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col < D) {
#pragma unroll
                    for (int i = 0; i < 8; i++) float_put(a.out, ffmt, eb + (uint64_t)(i * D + col), float_value(v[i][k], fsb, fsc[k], fof[k]));
                }
            }
        } else if constexpr (Q == kQueryProject) {
            // the selected columns' samples, each at its slot of its output row (out_elems + blk_elems <= chunk_len: checked above, so the
            // rows lie inside the chunk's R); 64-bit addresses, so this kernel takes every layout, every K and every alignment of the output
            (void)ob;
            const uint64_t rb = prow0 + out_elems / (uint32_t)D;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                if (pslot[k] < pK) {
#pragma unroll
                    for (int i = 0; i < 8; i++) project_put<W>(a, (rb + (uint64_t)i) * (uint64_t)pK + pslot[k], v[i][k], pslot[k]);
                }
            }
        } else if (cs) {
            const uint32_t r0 = out_elems / (uint32_t)D;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col < D) {
                    U* const cp = cm0 + (uint64_t)col * cs + r0;
#pragma unroll
                    for (int i = 0; i < 8; i++) cp[i] = (U)v[i][k];
                }
            }
        } else if (LOWDIM && D == 1) {
            // one column: the block's 8 samples are contiguous -- one store, not eight
            if (lane_d == 0) {
                typedef uint32_t v2 __attribute__((ext_vector_type(2)));
                typedef uint32_t v4 __attribute__((ext_vector_type(4)));
                typedef v2 __attribute__((aligned(1), may_alias)) v2u;
                typedef v4 __attribute__((aligned(1), may_alias)) v4u;
                if constexpr (W == 8) {
                    v2 t;
                    t.x = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[3][0] << 24);
                    t.y = v[4][0] | (v[5][0] << 8) | (v[6][0] << 16) | (v[7][0] << 24);
                    *(v2u*)ob = t;
                } else {
                    v4 t;
                    t.x = v[0][0] | (v[1][0] << 16);
                    t.y = v[2][0] | (v[3][0] << 16);
                    t.z = v[4][0] | (v[5][0] << 16);
                    t.w = v[6][0] | (v[7][0] << 16);
                    *(v4u*)ob = t;
                }
            }
        } else if (a.vec_store) {
            U* const l = (U*)lds;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col < D) {
#pragma unroll
                    for (int i = 0; i < 8; i++) l[i * D + col] = (U)v[i][k];
                }
            }
            wave_lds_sync();
            const uint32_t nunits = (blk_elems * ESZ) >> 4;
            for (uint32_t u = (uint32_t)lane_d; u < nunits; u += (uint32_t)DP)
                ((uint4*)ob)[u] = ((const uint4*)lds)[u];
            wave_lds_sync();
        } else {
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col < D) {
#pragma unroll
                    for (int i = 0; i < 8; i++) ob[i * D + col] = (U)v[i][k];
                }
            }
        }
        out_elems += blk_elems;
    }

    // ---- verbatim tail (:1171)
    if (!corrupt && (out_elems + remaining > a.chunk_len || (uint64_t)remaining * ESZ > (uint64_t)(stream_len - pos))) corrupt = true;
    if constexpr (Q == kQueryFilter) {
        if (!corrupt) filter_tail<W, CPL>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / blk_elems, lane_d, DP, fc, colk, genk, fcnt);
        if (lane_d == 0 && a.filter.counts) a.filter.counts[chunk] = fcnt;
    } else if constexpr (LIN) {
        if (!corrupt) linear_tail<W, CPL>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / blk_elems, lane_d, DP, lc, colk, genk, lctx, lcarry, pv, fcnt);
        else linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
        if (lane_d == 0 && a.filter.counts) a.filter.counts[chunk] = fcnt;
    } else if constexpr (Q == kQueryWindow) {
        if (!corrupt) window_tail<W, CPL>(a, s + pos, remaining, (uint32_t)D, colk, genk, wbase, wi, wleft, qmin, qmax, qsum);
    } else if constexpr (Q == kQueryAggregate) {
        if (!corrupt) aggregate_tail<W, CPL>(a, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk, wbase, wi, wleft, qmin, qmax, qsum, acnt, lane_d,
                                             [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (SEG) {
        if (!corrupt) segment_tail<W, CPL>(a, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk, sst, sbase, grow0, qmin, qmax, qsum, lane_d,
                                           [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (MOM) {
        if (!corrupt) moments_tail<W, CPL>(a, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk, wbase, wi, wleft, macc, acnt, lane_d,
                                           [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (EXT) {
        if (!corrupt) extrema_tail<W, CPL>(a, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk, wbase, wi, wleft, eacc, erows, acnt, lane_d,
                                           [&](uint32_t b) { return (uint32_t)smb[b]; });
    } else if constexpr (Q == kQueryMaterialize || Q == kQueryReduceOnly) {
        if (!corrupt) reduce_tail<W, CPL>(a, chunk, s + pos, remaining, (uint32_t)D, colk, genk, qmax, qsum);      // (out_elems is a multiple of 8*D)
    }
    if constexpr (HIST) {
        if (!corrupt) hist_tail<W, CPL>(a, hctx, hcol, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk,
                                        [&](uint32_t b) { return (uint32_t)smb[b]; });
        if (hlive && lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        hist_end(a, hctx);
        return;
    }
    if constexpr (GBY) {
        if (!corrupt) groupby_tail<W, CPL>(a, gctx, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, colk, genk, lane_d,
                                           [&](uint32_t b) { return (uint32_t)smb[b]; });
        if (hlive && lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        groupby_end(a, gctx);
        return;
    }
    if constexpr (Q == kQueryGather) {
        gather_tail<W>(a, gp, s + pos, out_elems, remaining, (uint32_t)D, lane_d, DP, corrupt, false);
        return;
    }
    if constexpr (Q == kQuerySelect) {
        if (!corrupt) select_tail<W>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, sbase, srank, lane_d, DP,
                                     [&](uint32_t b) { return (uint32_t)smb[b]; });
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (ROLL) {
        if (!corrupt) rolling_tail<W, CPL>(a, chunk, lds + a.table.table_off, s + pos, out_elems, remaining, (uint32_t)D, colk, genk, rsum);
        rolling_leave<W, CPL>(a, chunk, lds + a.table.table_off, corrupt ? 0u : out_elems + remaining, (uint32_t)D, colk, genk, lane_d);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (FIR) {
        if (!corrupt) fir_tail<W, CPL>(a, chunk, lds + a.table.table_off, s + pos, out_elems, remaining, (uint32_t)D, colk, genk);
        fir_leave<W, CPL>(a, chunk, lds + a.table.table_off, corrupt ? 0u : out_elems + remaining, (uint32_t)D, colk, genk, lane_d);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (CUM) {
        if (!corrupt) cumulative_tail<W, CPL>(a, chunk, s + pos, out_elems, remaining, (uint32_t)D, colk, genk, cst);
        cumulative_leave<W, CPL>(a, chunk, corrupt, (uint32_t)D, colk, genk, cst);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (DER) {
        if (!corrupt) derive_tail<W, CPL>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / blk_elems, lane_d, DP, colk, genk, dlast);
        else linear_mark(a, chunk, (uint32_t)D, W, 0u, lane_d);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (Q == kQueryFloat) {
        if (!corrupt) float_tail<W>(a, chunk, s + pos, out_elems, remaining, (uint32_t)D, lane_d, DP);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if constexpr (Q == kQueryProject) {
        if (!corrupt) project_tail<W>(a, chunk, s + pos, out_elems, remaining, (uint32_t)D, lane_d, DP);
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if (!corrupt && !query_reduce_only(Q) && cs) {
        const uint8_t* t = s + pos;
        const uint32_t r0 = out_elems / (uint32_t)D;
        for (uint32_t e = (uint32_t)lane_d; e < remaining; e += (uint32_t)DP) {
            const uint32_t x = tail_elem<W>(t, e);
            cm0[(uint64_t)(e % (uint32_t)D) * cs + r0 + e / (uint32_t)D] = (U)x;
        }
    } else if (!corrupt && !query_reduce_only(Q)) {
        const uint8_t* t = s + pos;
        uint8_t* d = (uint8_t*)(o + out_elems);
        copy_verbatim(t, d, remaining * ESZ, (uint32_t)lane_d, (uint32_t)DP);
    }
    if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
}

}  // namespace sprintz
