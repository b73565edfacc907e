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

#include "sprintz_device.h"

namespace sprintz {

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
    // query-on-compressed (sprintz_delta.h:95-98, sprintz_xff.h:90-93, query.hpp:23-29): kernels
    // instantiated with Q != 0 reduce every column of every chunk while decoding
    // column-major destination (BASELINE config 5): element (row r, column d) at out[d*col_stride + r];
    // chunk c holds rows [c*chunk_len/D, ...).  0 = row-major.
    uint64_t col_stride;
    // non-RLE codecs (sprintz_delta.cpp:64-1391; generic kernel only): 6-byte header {u32 len; u16 ndims},
    // len/(16 D) groups, an all-zero block has no payload and no run length; raw: bit-packing only
    int norle;
    int raw;
    int quirk;                  // 1: replay the runs of 16-bit general-layout FIRE streams as the REFERENCE DECODER does (fire_coef_ref_run16)
    int qop;                    // 1: max, 2: sum (what lands in qres)
    uint64_t* qres;             // [nchunks][D] per-chunk, per-column partial results
    // a single call on the caller thread's mapped host buffer (decode_lat.h alone): offsets == null -> the one chunk's stream is
    // comp[one_off0, one_off1); host_flag != null -> the kernel ends by writing host_ticket there, after every lane's stores
    uint64_t one_off0, one_off1;
    uint64_t* host_flag;
    uint64_t host_ticket;
    // windowed query (Q == kQueryWindow; sprintz_mi355x_query_windows): chunk c, window w (rows [w*W, (w+1)*W) of the chunk
    // slot) and column d land at entry (c*win_count + w)*D + d of each selected output; appended so that no field above moves
    uint32_t window_rows;       // W, a multiple of 8: a block of 8 rows never straddles a window edge
    uint32_t win_count;         // windows per chunk slot: ceil(ceil(chunk_len / D) / W)
    uint32_t win_ops;           // SPRINTZ_QUERY_WIN_MIN 1 | _MAX 2 | _SUM 4
    void* win_min;              // element type
    void* win_max;              // element type
    uint64_t* win_sum;
    // gather rows (Q == kQueryGather; sprintz_mi355x_gather_rows): range i is batch rows [g_starts[i], g_starts[i] + g_rows), batch row g
    // being row g % g_rpc of chunk g / g_rpc; piece slot s = i * g_pieces + k decodes chunk g_starts[i] / g_rpc + k (gather_piece below)
    const uint64_t* g_starts;   // [g_nranges], on the device
    uint64_t g_nranges;
    uint32_t g_rows;            // rows of every range
    uint32_t g_rpc;             // R: rows of a chunk slot, chunk_len / D
    uint32_t g_pieces;          // P: the most chunks a range can touch, (g_rows + R - 2) / R + 1
    // filter rows (Q == kQueryFilter; sprintz_mi355x_filter_rows): row r of chunk c matches if every (f_mode 0) / some (f_mode 1) column d
    // has f_lo[d] <= x <= f_hi[d], unsigned; bit r & 7 of f_mask[c * f_mask_stride + (r >> 3)], the chunk's matches in f_counts[c]
    const void* f_lo;           // [D], element type, on the device
    const void* f_hi;
    uint32_t f_mode;            // SPRINTZ_FILTER_ALL 0 / SPRINTZ_FILTER_ANY 1: wave-uniform, not a template parameter
    uint8_t* f_mask;            // optional
    uint32_t* f_counts;         // optional
    uint32_t f_mask_stride;     // MB: mask bytes of a chunk slot, ceil(ceil(chunk_len / D) / 8)
    // select rows (Q == kQuerySelect; sprintz_mi355x_select_rows): the i-th set bit of chunk c's mask bytes s_mask[c * f_mask_stride ...]
    // (filter_rows' layout), row r, lands at row s_bases[c] + i of `out` and c * g_rpc + r at the same place of s_ids; a place
    // >= s_capacity is dropped
    const uint8_t* s_mask;      // [nchunks][f_mask_stride]
    const uint64_t* s_bases;    // [nchunks]
    uint64_t s_capacity;        // rows of `out` (and entries of s_ids)
    uint64_t* s_ids;            // optional
};

// select rows: the places of the rows of one 8-row block (or of 8 rows of the tail) whose bits are set in m, behind `first` -- the
// chunk's base plus the set bits in front of the block
__device__ __forceinline__ uint64_t select_place(uint64_t first, uint32_t m, uint32_t row) { return first + (uint32_t)__popc(m & ((1u << row) - 1u)); }
// the row numbers of those rows: lanes 0 .. 7 of the group take a row each (groups of fewer lanes take turns); one writer an entry
__device__ __forceinline__ void select_ids(const DecodeArgs& a, uint64_t first, uint32_t m, uint64_t row0, int lane_d, int DP)
{
    if (!a.s_ids) return;
    for (uint32_t j = (uint32_t)lane_d; j < 8u; j += (uint32_t)DP) {
        const uint64_t p = select_place(first, m, j);
        if (((m >> j) & 1u) && p < a.s_capacity) a.s_ids[p] = row0 + j;
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
    constexpr int ESZ = W / 8;
    typedef uint16_t __attribute__((aligned(1), may_alias)) u16u;
    const uint32_t nfull = remaining / D;
    for (uint32_t r0 = 0; r0 < nfull; r0 += 8u) {
        const uint32_t n = nfull - r0 < 8u ? nfull - r0 : 8u;
        const uint32_t m = mask_at((row0 + r0) >> 3) & ((1u << n) - 1u);
        const uint64_t first = base + rank;
        for (uint32_t j = 0; j < n; j++) {
            if (!((m >> j) & 1u)) continue;
            const uint64_t p = select_place(first, m, j);
            if (p >= a.s_capacity) continue;
            U* const d = (U*)a.out + p * (uint64_t)D;
            const uint8_t* const s = t + (size_t)(r0 + j) * D * ESZ;
            for (uint32_t e = (uint32_t)lane_d; e < D; e += (uint32_t)DP) d[e] = ESZ == 1 ? (U)s[e] : (U)*(const u16u*)(s + 2 * e);
        }
        select_ids(a, first, m, chunk * (uint64_t)a.g_rpc + row0 + r0, lane_d, DP);
        rank += (uint32_t)__popc(m);
    }
}

// windowed query: one column's entries of one window leave (each entry has exactly one writer -- no atomics), and the
// accumulators start over from the identities (min = all ones, max = 0, sum = 0)
template <int W>
__device__ __forceinline__ void win_flush(const DecodeArgs& a, uint64_t idx, uint32_t& qmin, uint32_t& qmax, uint64_t& qsum)
{
    using U = typename Elem<W>::U;
    if (a.win_ops & 1u) ((U*)a.win_min)[idx] = (U)qmin;
    if (a.win_ops & 2u) ((U*)a.win_max)[idx] = (U)qmax;
    if (a.win_ops & 4u) a.win_sum[idx] = qsum;
    qmin = Elem<W>::MASK;
    qmax = 0;
    qsum = 0;
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
        const uint32_t lo = ((const U*)a.f_lo)[col], hi = ((const U*)a.f_hi)[col];
        f.lo = lo;
        f.span = lo <= hi ? hi - lo + 1u : 0u;
    }
    return f;
}
// (x may carry garbage above bit W: only its low W bits reach the masked difference)
template <int W> __device__ __forceinline__ uint32_t filter_hit(const FilterCol& f, uint32_t x) { return ((x - f.lo) & Elem<W>::MASK) < f.span ? 1u : 0u; }
__device__ __forceinline__ uint32_t filter_inv(const DecodeArgs& a) { return a.f_mode == 0u ? 0xffffffffu : 0u; }
__device__ __forceinline__ uint32_t group_or_any(uint32_t v, int DP)
{
    for (int off = DP >> 1; off > 0; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, DP);
    return v;
}
// The verbatim tail, for the lane-per-column kernels: `remaining` elements at t, row-major from the row behind the chunk's
// `blocks_done` blocks.  A partial last row is not a row.  32 rows a trip: a lane folds its columns into one word, the group ORs
// the words, lanes 0 .. 3 store the trip's bytes; then the mask bytes of the slot's rows past the data are zeroed, spread over the
// lanes.  Every byte has one writer, and all of them lie in the chunk's f_mask_stride bytes: blocks_done * 8 + remaining / D rows
// are at most chunk_len / D (the callers check the tail against the slot before they come here).
template <int W, int CPL>
__device__ __forceinline__ void filter_tail(const DecodeArgs& a, uint64_t chunk, const uint8_t* t, uint32_t remaining, uint32_t D, uint32_t blocks_done,
                                            int lane_d, int DP, const FilterCol (&fc)[CPL], const int (&col)[CPL], const bool (&genuine)[CPL], uint32_t& count)
{
    constexpr int ESZ = W / 8;
    typedef uint16_t __attribute__((aligned(1), may_alias)) u16u;   // the tail starts at any byte: one 2-byte load an element
    const uint32_t nfull = remaining / D, tbytes = (nfull + 7u) >> 3;
    const uint32_t inv = filter_inv(a);
    uint8_t* const mb = a.f_mask ? a.f_mask + chunk * (uint64_t)a.f_mask_stride : nullptr;
    for (uint32_t r0 = 0; r0 < nfull; r0 += 32u) {
        const uint32_t n = nfull - r0 < 32u ? nfull - r0 : 32u;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            if (!genuine[k]) continue;
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t e = (r0 + j) * D + (uint32_t)col[k];
                const uint32_t x = ESZ == 1 ? (uint32_t)t[e] : (uint32_t)*(const u16u*)(t + 2 * e);
                v |= (filter_hit<W>(fc[k], x) ^ (inv & 1u)) << j;
            }
        }
        v = (group_or_any(v, DP) ^ inv) & (n == 32u ? 0xffffffffu : (1u << n) - 1u);
        count += (uint32_t)__popc(v);
        if (mb) {
            for (uint32_t b = (uint32_t)lane_d; b < 4u; b += (uint32_t)DP)
                if ((r0 >> 3) + b < tbytes) mb[blocks_done + (r0 >> 3) + b] = (uint8_t)(v >> (8u * b));
        }
    }
    if (mb) {
        for (uint32_t j = blocks_done + tbytes + (uint32_t)lane_d; j < a.f_mask_stride; j += (uint32_t)DP) mb[j] = 0;
    }
}

constexpr int64_t kErrCorrupt = -5;
constexpr int64_t kErrNoRow = -1;             // gather: the range needs a row that does not exist (SPRINTZ_E_INVALID)

// gather: what piece slot `slot` has to do.  All of it follows from g_starts[range] on the device; a slot past the range's last
// chunk has nothing to do (false).  `obase` is where row 0 of the piece's CHUNK would land in `out`, in elements: negative or past
// the range's own rows for most pieces -- the row test [lo, hi) alone decides which stores happen.
struct GatherPiece {
    uint64_t range, chunk;
    uint32_t lo, hi;            // chunk-relative rows the range needs from this chunk, lo < hi <= g_rpc
    int64_t obase;
    bool exists;                // chunk < nchunks; if not, the range fails without a decode
};
__device__ __forceinline__ bool gather_piece(const DecodeArgs& a, uint64_t slot, GatherPiece& p)
{
    p.range = slot / a.g_pieces;
    if (p.range >= a.g_nranges) return false;
    const uint64_t k = slot - p.range * a.g_pieces, R = a.g_rpc;
    const uint64_t g0 = a.g_starts[p.range], c0 = g0 / R;
    p.exists = c0 < a.nchunks;                      // (checked first: c0 + k cannot wrap below)
    p.chunk = 0; p.lo = 0; p.hi = 1; p.obase = 0;
    if (!p.exists) return k == 0;                   // one slot reports the missing rows
    const uint64_t first = g0 - c0 * R, end = first + a.g_rows;   // the range, in rows from row 0 of chunk c0
    if (k * R >= end) return false;
    p.chunk = c0 + k;
    p.exists = p.chunk < a.nchunks;
    p.lo = (uint32_t)((first > k * R ? first : k * R) - k * R);
    p.hi = (uint32_t)((end < (k + 1) * R ? end : (k + 1) * R) - k * R);
    p.obase = ((int64_t)(p.range * a.g_rows) + (int64_t)(k * R) - (int64_t)first) * (int64_t)a.D;
    return true;
}
// a failing piece leaves its code in the range's entry (the entries start at g_rows: gather_rets_fill; the smallest code wins)
__device__ __forceinline__ void gather_fail(const DecodeArgs& a, uint64_t range, int64_t code)
{
    if (a.rets) atomicMin((long long*)&a.rets[range], (long long)code);
}

template <int W, bool FIRE, bool LOWDIM, int CPL, int Q = 0>
__global__ void __launch_bounds__(kThreads) decode_kernel(DecodeArgs a)
{
    using U = typename Elem<W>::U;
    constexpr int HB = Elem<W>::HB;
    constexpr uint32_t MASK = Elem<W>::MASK;
    constexpr int ESZ = W / 8;
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
    const uint64_t chunk = chunk_sel;
    if (chunk >= a.nchunks) return;                 // whole groups leave together

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
    if (a.norle) {                                   // format.h:65-86; sprintz_delta.cpp:803-807, :832
        // norle == 2: compress8b_rowmajor_xff's 8-byte header, a u64 len whose bytes 6..7 hold ndims (sprintz_xff.cpp:58-63)
        const uint32_t len = load_u32_any(s);
        const uint32_t ndo = a.norle == 2 ? 6u : 4u;
        const uint32_t nd = load_u8(s + ndo) | (load_u8(s + ndo + 1) << 8);
        if ((int)nd != D || len > a.chunk_len) {
            if constexpr (Q == kQueryGather) { if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt); }
            else if (lane_d == 0 && a.rets) a.rets[chunk] = kErrCorrupt;
            return;
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
            return;
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
    uint32_t qmax[CPL];
    uint64_t qsum[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) { qmax[k] = 0; qsum[k] = 0; }
    // windowed query: the window being accumulated and the rows it still takes
    // (set up in that mode alone: the other instantiations stay exactly as they were)
    uint32_t qmin[CPL];
    uint32_t wi = 0, wleft = 0;
    uint64_t wbase = 0;
    if constexpr (Q == kQueryWindow) {
#pragma unroll
        for (int k = 0; k < CPL; k++) qmin[k] = MASK;
        wleft = a.window_rows;
        wbase = chunk * (uint64_t)a.win_count;
    }
    // filter rows: each lane's columns' bounds, loaded once; the group ORs its lanes' block masks with wave shuffles (groups of up to
    // 64 lanes, both layouts), lane 0 stores the block's byte -- runs are replayed block by block here, as the decode does
    FilterCol fc[CPL];
    int fcol[CPL];
    bool fgen[CPL];
    uint32_t finv = 0, fcnt = 0;
    uint8_t* fmb = nullptr;
    if constexpr (Q == kQueryFilter) {
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            fcol[k] = lane_d * CPL + k;
            fgen[k] = fcol[k] < D;
            fc[k] = filter_col<W>(a, fcol[k], fgen[k]);
        }
        finv = filter_inv(a);
        if (a.f_mask) fmb = a.f_mask + chunk * (uint64_t)a.f_mask_stride;
    }

    // select rows: the chunk's mask bytes, its first output row and the set bits of the blocks done so far
    const uint8_t* smb = nullptr;
    uint64_t sbase = 0;
    uint32_t srank = 0;
    if constexpr (Q == kQuerySelect) {
        smb = a.s_mask + chunk * (uint64_t)a.f_mask_stride;
        sbase = a.s_bases[chunk];
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
                fl |= fgen[k] ? (cm ^ finv) & 0xffu : 0u;
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
        if constexpr (Q == kQueryWindow) {       // the block's 8 rows lie in one window: flush it when they complete it
            wleft -= 8;
            if (wleft == 0) {
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    const int col = lane_d * CPL + k;
                    if (col < D) win_flush<W>(a, (wbase + wi) * (uint64_t)D + (uint64_t)col, qmin[k], qmax[k], qsum[k]);
                }
                wi++;
                wleft = a.window_rows;
            }
        }

        if constexpr (Q == kQueryFilter) {       // block out_elems / blk_elems < chunk_len / blk_elems <= f_mask_stride (checked above)
            const uint32_t m = (group_or_any(fl, DP) ^ finv) & 0xffu;
            if (fmb && lane_d == 0) fmb[out_elems / blk_elems] = (uint8_t)m;
            fcnt += (uint32_t)__popc(m);
        }

        // ---- store the 8 x D block (contiguous 8*D*ESZ bytes of the output)
        U* const ob = o + out_elems;
        if constexpr (query_reduce_only(Q)) {
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
            if (r0 + 8u >= gp.hi) return;            // delivered in full: the range's entry keeps g_rows
        } else if constexpr (Q == kQuerySelect) {
            // the block's rows whose bits are set, each at its place behind the chunk's base (block out_elems / blk_elems <
            // chunk_len / blk_elems <= f_mask_stride: checked above); 64-bit addresses, a place >= s_capacity is dropped
            (void)ob;
            const uint32_t r0 = out_elems / (uint32_t)D;
            const uint32_t m = smb[r0 >> 3];
            const uint64_t first = sbase + srank;
            if (m) {
#pragma unroll
                for (int k = 0; k < CPL; k++) {
                    const int col = lane_d * CPL + k;
                    if (col < D) {
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const uint64_t p = select_place(first, m, (uint32_t)i);
                            if (((m >> i) & 1u) && p < a.s_capacity) ((U*)a.out)[p * (uint64_t)D + (uint64_t)col] = (U)v[i][k];
                        }
                    }
                }
                select_ids(a, first, m, chunk * (uint64_t)a.g_rpc + r0, lane_d, DP);
            }
            srank += (uint32_t)__popc(m);
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
        if (!corrupt) filter_tail<W, CPL>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / blk_elems, lane_d, DP, fc, fcol, fgen, fcnt);
        if (lane_d == 0 && a.f_counts) a.f_counts[chunk] = fcnt;
    } else if constexpr (Q == kQueryWindow) {
        // tail element e is in column e % D, one row further on than the column's previous one; a window
        // edge can fall inside the tail.  Then the partial window and the identities of the slot's last ones.
        if (!corrupt) {
            const uint8_t* t = s + pos;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col >= D) continue;
                uint32_t w = wi, left = wleft;
                for (uint32_t e = (uint32_t)col; e < remaining; e += (uint32_t)D) {
                    if (left == 0) {
                        win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)col, qmin[k], qmax[k], qsum[k]);
                        w++;
                        left = a.window_rows;
                    }
                    left--;
                    const uint32_t x = ESZ == 1 ? load_u8(t + e) : (load_u8(t + 2 * e) | (load_u8(t + 2 * e + 1) << 8));
                    qmin[k] = x < qmin[k] ? x : qmin[k];
                    qmax[k] = x > qmax[k] ? x : qmax[k];
                    qsum[k] += x;
                }
                for (; w < a.win_count; w++) win_flush<W>(a, (wbase + w) * (uint64_t)D + (uint64_t)col, qmin[k], qmax[k], qsum[k]);
            }
        }
    } else if constexpr (Q != 0) {
        // the verbatim tail continues the row-major order: element e sits in column e % D
        // (out_elems is a multiple of 8*D)
        if (!corrupt) {
            const uint8_t* t = s + pos;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const int col = lane_d * CPL + k;
                if (col >= D) continue;
                for (uint32_t e = (uint32_t)col; e < remaining; e += (uint32_t)D) {
                    const uint32_t x = ESZ == 1 ? load_u8(t + e) : (load_u8(t + 2 * e) | (load_u8(t + 2 * e + 1) << 8));
                    qmax[k] = x > qmax[k] ? x : qmax[k];
                    qsum[k] += x;
                }
                if (a.qres) a.qres[chunk * (uint64_t)D + (uint64_t)col] = a.qop == 1 ? (uint64_t)qmax[k] : qsum[k];
            }
        }
    }
    if constexpr (Q == kQueryGather) {
        // the piece still needs rows of the verbatim tail -- or rows the stream does not hold (the short last chunk)
        if (!corrupt && (uint64_t)gp.hi * (uint32_t)D > (uint64_t)out_elems + remaining) {
            if (lane_d == 0) gather_fail(a, gp.range, kErrNoRow);
            return;
        }
        if (corrupt) {
            if (lane_d == 0) gather_fail(a, gp.range, kErrCorrupt);
            return;
        }
        const uint8_t* t = s + pos;
        const uint32_t e_lo = gp.lo * (uint32_t)D > out_elems ? gp.lo * (uint32_t)D - out_elems : 0u;
        const uint32_t e_hi = gp.hi * (uint32_t)D - out_elems;                  // <= remaining, checked above
        for (uint32_t e = e_lo + (uint32_t)lane_d; e < e_hi; e += (uint32_t)DP) {
            const uint32_t x = ESZ == 1 ? load_u8(t + e) : (load_u8(t + 2 * e) | (load_u8(t + 2 * e + 1) << 8));
            ((U*)a.out)[gp.obase + (int64_t)out_elems + (int64_t)e] = (U)x;
        }
        return;
    }
    if constexpr (Q == kQuerySelect) {
        if (!corrupt) select_tail<W>(a, chunk, s + pos, remaining, (uint32_t)D, out_elems / (uint32_t)D, sbase, srank, lane_d, DP,
                                     [&](uint32_t b) { return (uint32_t)smb[b]; });
        if (lane_d == 0 && a.rets) a.rets[chunk] = corrupt ? kErrCorrupt : (int64_t)out_elems + remaining;
        return;
    }
    if (!corrupt && !query_reduce_only(Q) && cs) {
        const uint8_t* t = s + pos;
        const uint32_t r0 = out_elems / (uint32_t)D;
        for (uint32_t e = (uint32_t)lane_d; e < remaining; e += (uint32_t)DP) {
            const uint32_t x = ESZ == 1 ? load_u8(t + e) : (load_u8(t + 2 * e) | (load_u8(t + 2 * e + 1) << 8));
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
