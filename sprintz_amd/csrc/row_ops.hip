// row_ops.hip -- the row operations of the C-ABI (include/sprintz_mi355x.h): queries, the zone map, filters, select, aggregate,
// moments, extrema, segments, float rows, rolling rows, project rows, derive rows, FIR rows, histogram, group-by and gather on a compressed batch.  Each entry point names its batch, runs its checks,
// fills its QuerySpec and hands over to decode_batch (entry.h); what the decoders then do with a row is decode_ops.h's.
#include "entry.h"

#include <string>

using namespace sprintz;

namespace {

// gather_rows: every range's entry starts at `rows`; a failing piece lowers it to its code (decode_ops.h: gather_fail)
__global__ void gather_rets_fill(int64_t* rets, uint64_t n, int64_t v)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rets[i] = v;
}

// what the row operations (query_windows, gather_rows, filter_rows, select_rows, aggregate_rows, histogram_rows, moments_rows, groupby_rows, extrema_rows, filter_linear) check alike, behind check_common; the refusals that
// name the operation come in its own words (rle_only == null: every codec is taken; op != null: its name in front of the shared ones)
int check_row_op(const Batch& b, uint32_t flags, const char* many_columns, const char* rle_only, const char* op = nullptr)
{
    if (flags & ~(uint32_t)SPRINTZ_QUERY_GENERAL_LAYOUT) return fail_op(SPRINTZ_E_INVALID, op, "unknown flag");
    if (b.chunk_len == 0 || b.chunk_len > (1u << 30)) return fail_op(SPRINTZ_E_INVALID, op, "chunk_len must be in 1..2^30");
    if (!b.comp || !b.offsets) return fail_op(SPRINTZ_E_INVALID, op, "null device pointer");
    if (b.ndims > 512) return fail(SPRINTZ_E_UNSUPPORTED, many_columns);
    if (rle_only && b.codec != SPRINTZ_CODEC_DELTA && b.codec != SPRINTZ_CODEC_XFF) return fail(SPRINTZ_E_UNSUPPORTED, rle_only);
    return 0;
}

// The outputs of an operation that selects them by the bits of `ops`, out[i] for bit i.  One counts only where its op is selected:
// the others may be NULL or lie anywhere, and are nulled here so that they reach the kernels as null -- not touched.  A selected one
// must be there and aligned (rets8, where the operation words d_rets' alignment into the same refusal: d_rets too).
// `misaligned`: the operation's own words; op != null: its name in front of both refusals
struct OpOutput { void* p; int align; };
template <int N>
int check_op_outputs(const char* op, uint32_t ops, OpOutput (&out)[N], const void* rets8, const char* misaligned)
{
    for (int i = 0; i < N; i++) {
        if (!(ops & (1u << i))) out[i].p = nullptr;
        else if (!out[i].p) return fail_op(SPRINTZ_E_INVALID, op, "a selected op without its output buffer");
    }
    bool bad = (uintptr_t)rets8 % 8 != 0;
    for (int i = 0; i < N; i++) bad = bad || (uintptr_t)out[i].p % (uintptr_t)out[i].align;
    return bad ? fail_op(SPRINTZ_E_INVALID, op, misaligned) : 0;
}

// a row operation's QuerySpec: its mode and the layout its flags ask for
QuerySpec row_query(int q, uint32_t flags)
{
    QuerySpec qs;
    qs.q = q;
    qs.general = (flags & SPRINTZ_QUERY_GENERAL_LAYOUT) ? 1 : 0;
    return qs;
}

// the refusals every one of them shares, and rolling rows, which takes every row and no mask: the common ones, whole rows a chunk
int unmasked_row_op(const char* op, const Batch& b, uint32_t flags)
{
    int rc = check_common(b.codec, b.esz, b.ndims);
    if (rc) return rc;
    const std::string many = std::string(op) + ": more than 512 columns", rle = std::string(op) + ": the RLE codecs (delta, xff) only";
    if ((rc = check_row_op(b, flags, many.c_str(), rle.c_str(), op))) return rc;
    if (b.chunk_len % b.ndims) return fail_op(SPRINTZ_E_INVALID, op, "chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    return 0;
}
// ---- what aggregate_rows, moments_rows, histogram_rows, groupby_rows and extrema_rows check and fill alike.  Each refusal carries the operation's
// name `op` (fail_op), and each helper is called where its refusals stand among the operation's own.
// the four masked operations, in front of their own checks: the common refusals, whole rows a chunk; then the mode, the layout and the
// row mask (null: every row, where the operation allows it)
int masked_row_op(const char* op, int q, const Batch& b, uint32_t flags, const uint8_t* d_mask, QuerySpec& qs)
{
    if (int rc = unmasked_row_op(op, b, flags)) return rc;
    qs = row_query(q, flags);
    qs.rows = RowMaskArgs{d_mask, (b.chunk_len / b.ndims + 7) / 8};
    return 0;
}
// the windowed three (aggregate, moments, extrema), behind masked_row_op: the windows of a chunk slot
int windowed_row_op(const char* op, uint32_t window_rows, const Batch& b, QuerySpec& qs)
{
    const uint32_t rows = b.chunk_len / b.ndims;
    if (window_rows < 8 || window_rows % 8) return fail_op(SPRINTZ_E_INVALID, op, "window_rows must be a multiple of 8, at least 8");
    qs.win.rows = window_rows;
    qs.win.count = (uint32_t)(((uint64_t)rows + window_rows - 1) / window_rows);      // (64 bits: rows + window_rows may pass 2^32)
    return 0;
}
// the binned pair (histogram, group-by): the bins ...
int binned_row_op(const char* op, int esz, uint32_t shift, uint32_t nbins)
{
    const uint32_t W = 8u * (uint32_t)esz;
    if (shift >= W) return fail_op(SPRINTZ_E_INVALID, op, "shift must be below the element width");
    if (nbins < 1 || nbins > (1u << (W - shift))) return fail_op(SPRINTZ_E_INVALID, op, "nbins must be in 1..2^(W - shift)");
    return 0;
}
// ... the tables of the outputs, span_chunks consecutive chunks each (0: one for the batch), ndims x nbins 64-bit entries the largest
// output of a table: at most 2^40 entries a call (`too_many`: the refusal, in the operation's words) ...
int binned_tables(uint64_t nchunks, uint64_t span_chunks, uint16_t ndims, uint32_t nbins, const char* too_many, uint64_t* ntables)
{
    *ntables = span_chunks ? (nchunks + span_chunks - 1) / span_chunks : 1;
    if (*ntables > (1ull << 40) / ((uint64_t)ndims * nbins)) return fail(SPRINTZ_E_INVALID, too_many);
    return 0;
}
// ... and the launch.  Planned first: a call the planner refuses leaves the outputs as they were; zero_outputs(st) then zeroes them on
// the stream, in front of the kernel that adds to them
template <typename Z>
int binned_launch(const Batch& b, int64_t* d_rets, hipStream_t st, const QuerySpec& qs, Z zero_outputs)
{
    const Plan p = plan_decode(decode_shape(b, nullptr, qs), snapshot());
    if (p.err) return fail(p.err, p.what);
    if (int rc = zero_outputs(st)) return rc;
    return decode_launch(p, b, nullptr, d_rets, st, qs);
}

// per-column reduction of the per-chunk partials.  A workgroup covers RB rows x D columns per
// pass (thread = (row r, column col): a row of partials is contiguous, so consecutive threads
// read consecutive words), folds its rows through LDS and issues ONE atomic per column --
// 64 K threads each doing their own atomic on 8 addresses took 166 us for 8 MB.
__global__ void __launch_bounds__(256) query_reduce_kernel(const uint64_t* partials, uint64_t nchunks, uint32_t D, int op,
                                                           unsigned long long* result)
{
    __shared__ unsigned long long acc[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t RB = D >= 256 ? 1u : 256u / D;
    const uint32_t r = D >= 256 ? 0u : tid / D;
    const bool active = r < RB;
    for (uint32_t col = D >= 256 ? tid : tid % D; col < D; col += 256) {
        unsigned long long v = 0;
        if (active) {
            for (uint64_t c = (uint64_t)blockIdx.x * RB + r; c < nchunks; c += (uint64_t)gridDim.x * RB) {
                const unsigned long long x = partials[c * D + col];
                v = op == 1 ? (x > v ? x : v) : v + x;
            }
        }
        if (RB > 1) {
            acc[tid] = v;
            __syncthreads();
            if (r == 0) {
                for (uint32_t q = 1; q < RB; q++) {
                    const unsigned long long x = acc[q * D + col];
                    v = op == 1 ? (x > v ? x : v) : v + x;
                }
            }
            __syncthreads();
        }
        if (r == 0) {
            if (op == 1) atomicMax(&result[col], v);
            else atomicAdd(&result[col], v);
        }
    }
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- query-on-compressed
int sprintz_mi355x_query_batch(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, int op, int materialize, uint32_t flags, void* d_out,
                               uint64_t* d_partials, int64_t* d_rets, void* hip_stream)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (op < 0 || op > 2) return fail(SPRINTZ_E_INVALID, "op must be 0 (none), 1 (max) or 2 (sum)");
    if (flags & ~(uint32_t)SPRINTZ_QUERY_GENERAL_LAYOUT) return fail(SPRINTZ_E_INVALID, "unknown flag");
    if (chunk_len == 0 || chunk_len > (1u << 30)) return fail(SPRINTZ_E_INVALID, "chunk_len must be in 1..2^30");
    if (!d_comp || !d_offsets) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if (materialize && !d_out) return fail(SPRINTZ_E_INVALID, "materialize without a destination");
    if (op && !d_partials) return fail(SPRINTZ_E_INVALID, "op without a result buffer");
    if ((rc = ensure_device())) return rc;
    QuerySpec qs = row_query(materialize ? (op ? kQueryMaterialize : kQueryOff) : kQueryReduceOnly, flags);
    qs.qop = op;
    qs.qres = op ? d_partials : nullptr;
    return decode_batch(Batch{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims}, d_out, d_rets, (hipStream_t)hip_stream, qs);
}

int sprintz_mi355x_query_windows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                 uint32_t chunk_len, uint16_t ndims, uint32_t window_rows, uint32_t ops, uint32_t flags,
                                 void* d_min, void* d_max, uint64_t* d_sum, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (window_rows < 8 || window_rows % 8) return fail(SPRINTZ_E_INVALID, "window_rows must be a multiple of 8, at least 8");
    if (ops < 1 || ops > 7) return fail(SPRINTZ_E_INVALID, "ops must be a non-empty OR of SPRINTZ_QUERY_WIN_MIN / _MAX / _SUM");
    static_assert(SPRINTZ_QUERY_WIN_MIN == 1u && SPRINTZ_QUERY_WIN_MAX == 2u && SPRINTZ_QUERY_WIN_SUM == 4u, "out[i] is op bit i");
    OpOutput out[3] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_sum, 8}};
    if ((rc = check_op_outputs(nullptr, ops, out, nullptr, "min / max must be aligned to the element size, sum to 8 bytes"))) return rc;
    if ((rc = check_row_op(b, flags, "more than 512 columns: no query", nullptr))) return rc;
    if ((rc = ensure_device())) return rc;
    const uint32_t rows = (chunk_len + ndims - 1) / ndims;
    QuerySpec qs = row_query(kQueryWindow, flags);
    qs.win.rows = window_rows;
    qs.win.count = (rows + window_rows - 1) / window_rows;
    qs.win.ops = ops;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.sum = (uint64_t*)out[2].p;
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- zone map (its consumers: zone.hip)
int sprintz_mi355x_zone_map(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks, uint32_t chunk_len,
                            uint16_t ndims, uint32_t flags, void* d_zmin, void* d_zmax, int64_t* d_zlen, void* hip_stream)
{
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (!d_zmin || !d_zmax || !d_zlen) return fail(SPRINTZ_E_INVALID, "zone_map: null device pointer");
    if ((uintptr_t)d_zlen % 8) return fail(SPRINTZ_E_INVALID, "zone_map: d_zlen must be aligned to 8 bytes");
    // one window a chunk: the rows of a chunk slot rounded up to the window's granule (an unusable chunk_len is query_windows' to refuse)
    const uint64_t rows = ((uint64_t)chunk_len + ndims - 1) / ndims, window = rows ? (rows + 7) / 8 * 8 : 8;
    return sprintz_mi355x_query_windows(codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims, (uint32_t)window,
                                        SPRINTZ_QUERY_WIN_MIN | SPRINTZ_QUERY_WIN_MAX, flags, d_zmin, d_zmax, nullptr, d_zlen, hip_stream);
}

// ---------------------------------------------------------------- filter rows
int sprintz_mi355x_filter_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const void* d_lo, const void* d_hi, uint32_t mode,
                               uint32_t flags, uint8_t* d_mask, uint32_t* d_counts, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if (mode != SPRINTZ_FILTER_ALL && mode != SPRINTZ_FILTER_ANY) return fail(SPRINTZ_E_INVALID, "filter_rows: mode must be SPRINTZ_FILTER_ALL or SPRINTZ_FILTER_ANY");
    if ((rc = check_row_op(b, flags, "more than 512 columns: no filter", "filter_rows: the RLE codecs (delta, xff) only"))) return rc;
    if (!d_lo || !d_hi) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if (!d_mask && !d_counts) return fail(SPRINTZ_E_INVALID, "filter_rows: neither a mask nor counts asked for");
    if ((uintptr_t)d_lo % (uintptr_t)elem_bytes || (uintptr_t)d_hi % (uintptr_t)elem_bytes)
        return fail(SPRINTZ_E_INVALID, "filter_rows: d_lo / d_hi must be aligned to the element size");
    if ((uintptr_t)d_counts % 4 || (uintptr_t)d_rets % 8) return fail(SPRINTZ_E_INVALID, "filter_rows: d_counts must be aligned to 4 bytes, d_rets to 8");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    const uint32_t rows = (chunk_len + ndims - 1) / ndims;
    QuerySpec qs = row_query(kQueryFilter, flags);
    qs.filter = FilterArgs{d_lo, d_hi, mode, d_mask, d_counts, (rows + 7) / 8};
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- linear filter rows
uint64_t sprintz_mi355x_filter_linear_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims)
{
    if ((elem_bytes != 1 && elem_bytes != 2) || ndims == 0 || ndims > 512 || nchunks == 0) return 0;
    const uint64_t stride = linear_tmp_stride(elem_bytes, ndims);
    return nchunks > (1ull << 62) / stride ? 0 : nchunks * stride;
}

int sprintz_mi355x_filter_linear(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                 uint32_t chunk_len, uint16_t ndims, const int32_t* d_weights, const int32_t* d_lag_weights,
                                 int32_t bias, int32_t lo, int32_t hi, uint32_t flags, void* d_tmp, uint8_t* d_mask, uint32_t* d_counts,
                                 int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if ((rc = check_row_op(b, flags, "more than 512 columns: no filter", "filter_linear: the RLE codecs (delta, xff) only"))) return rc;
    if (!d_weights) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if (!d_mask && !d_counts) return fail(SPRINTZ_E_INVALID, "filter_linear: neither a mask nor counts asked for");
    if (chunk_len % ndims) return fail(SPRINTZ_E_INVALID, "filter_linear: chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if ((uintptr_t)d_weights % 4 || (uintptr_t)d_lag_weights % 4) return fail(SPRINTZ_E_INVALID, "filter_linear: d_weights / d_lag_weights must be aligned to 4 bytes");
    if ((uintptr_t)d_counts % 4 || (uintptr_t)d_rets % 8) return fail(SPRINTZ_E_INVALID, "filter_linear: d_counts must be aligned to 4 bytes, d_rets to 8");
    if (d_lag_weights && (!d_tmp || (uintptr_t)d_tmp % 8))
        return fail(SPRINTZ_E_INVALID, "filter_linear: with d_lag_weights, d_tmp must hold sprintz_mi355x_filter_linear_tmp_bytes bytes, aligned to 8");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    const uint32_t rows = chunk_len / ndims;
    QuerySpec qs = row_query(kQueryLinear, flags);
    qs.filter = FilterArgs{nullptr, nullptr, 0u, d_mask, d_counts, (rows + 7) / 8};
    qs.lin = LinearArgs{d_weights, d_lag_weights, d_lag_weights ? d_tmp : nullptr, lo, hi, bias, 0u};
    rc = decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
    if (rc || !d_lag_weights || nchunks < 2) return rc;
    // the seam pass, behind the decode on the same stream: row 0 of every chunk behind the first takes its true predecessor
    DecodeArgs a{};
    a.nchunks = nchunks;
    a.D = ndims;
    a.filter = qs.filter;
    a.lin = qs.lin;
    if (launch_linear_seam(elem_bytes, a, (hipStream_t)hip_stream) != hipSuccess) return fail(SPRINTZ_E_HIP, "filter_linear seam kernel launch");
    return 0;
}

int sprintz_mi355x_filter_row_ids(const uint8_t* d_mask, const uint64_t* d_bases, uint64_t nchunks, uint32_t chunk_len,
                                  uint16_t ndims, uint64_t* d_ids, uint64_t capacity, void* hip_stream)
{
    if (ndims == 0 || chunk_len == 0 || chunk_len > (1u << 30)) return fail(SPRINTZ_E_INVALID, "filter_row_ids: ndims == 0 or chunk_len outside 1..2^30");
    if (chunk_len % ndims) return fail(SPRINTZ_E_INVALID, "filter_row_ids: chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if (nchunks > 0 && (!d_mask || !d_bases || !d_ids)) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if ((uintptr_t)d_bases % 8 || (uintptr_t)d_ids % 8) return fail(SPRINTZ_E_INVALID, "filter_row_ids: d_bases and d_ids must be aligned to 8 bytes");
    if (nchunks == 0) return 0;
    int rc = ensure_device();
    if (rc) return rc;
    if (launch_filter_row_ids(d_mask, d_bases, nchunks, chunk_len / ndims, d_ids, capacity, (hipStream_t)hip_stream) != hipSuccess)
        return fail(SPRINTZ_E_HIP, "filter_row_ids kernel launch");
    return 0;
}

// ---------------------------------------------------------------- select rows
int sprintz_mi355x_select_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, const uint64_t* d_bases,
                               uint64_t capacity, uint32_t flags, void* d_out, uint64_t* d_ids, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if ((rc = check_row_op(b, flags, "more than 512 columns: no select", "select_rows: the RLE codecs (delta, xff) only"))) return rc;
    if (chunk_len % ndims) return fail(SPRINTZ_E_INVALID, "select_rows: chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if (!d_mask || !d_bases || !d_out) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if ((uintptr_t)d_out % (uintptr_t)elem_bytes) return fail(SPRINTZ_E_INVALID, "select_rows: d_out must be aligned to the element size");
    if ((uintptr_t)d_bases % 8 || (uintptr_t)d_ids % 8 || (uintptr_t)d_rets % 8)
        return fail(SPRINTZ_E_INVALID, "select_rows: d_bases, d_ids and d_rets must be aligned to 8 bytes");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    const uint32_t rows = chunk_len / ndims;
    QuerySpec qs = row_query(kQuerySelect, flags);
    qs.select = SelectArgs{d_bases, capacity, d_ids, rows};
    qs.rows = RowMaskArgs{d_mask, (rows + 7) / 8};
    return decode_batch(b, d_out, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- aggregate rows
int sprintz_mi355x_aggregate_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                  uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t window_rows, uint32_t ops,
                                  uint32_t flags, void* d_min, void* d_max, uint64_t* d_sum, uint32_t* d_count, int64_t* d_rets,
                                  void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("aggregate_rows", kQueryAggregate, b, flags, d_mask, qs);
    if (rc) return rc;
    if ((rc = windowed_row_op("aggregate_rows", window_rows, b, qs))) return rc;
    if (ops < 1 || ops > 15) return fail(SPRINTZ_E_INVALID, "aggregate_rows: ops must be a non-empty OR of SPRINTZ_AGG_MIN / _MAX / _SUM / _COUNT");
    if (!d_mask) return fail(SPRINTZ_E_INVALID, "aggregate_rows: null device pointer");
    static_assert(SPRINTZ_AGG_MIN == 1u && SPRINTZ_AGG_MAX == 2u && SPRINTZ_AGG_SUM == 4u && SPRINTZ_AGG_COUNT == 8u, "out[i] is op bit i");
    OpOutput out[4] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_sum, 8}, {d_count, 4}};
    if ((rc = check_op_outputs("aggregate_rows", ops, out, d_rets, "min / max must be aligned to the element size, count to 4 bytes, sum and d_rets to 8"))) return rc;
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    qs.win.ops = ops & 7u;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.sum = (uint64_t*)out[2].p;
    qs.win.row_count = (uint32_t*)out[3].p;
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- moments rows
int sprintz_mi355x_moments_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t window_rows,
                                uint32_t ops, uint32_t ref_col, uint32_t flags, uint32_t* d_count, uint64_t* d_sum,
                                uint64_t* d_sumsq, uint64_t* d_cross, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("moments_rows", kQueryMoments, b, flags, d_mask, qs);
    if (rc) return rc;
    if ((rc = windowed_row_op("moments_rows", window_rows, b, qs))) return rc;
    if (ops < 1 || ops > 15) return fail(SPRINTZ_E_INVALID, "moments_rows: ops must be a non-empty OR of SPRINTZ_MOM_COUNT / _SUM / _SUMSQ / _CROSS");
    static_assert(SPRINTZ_MOM_COUNT == 1u && SPRINTZ_MOM_SUM == 2u && SPRINTZ_MOM_SUMSQ == 4u && SPRINTZ_MOM_CROSS == 8u, "out[i] is op bit i");
    OpOutput out[4] = {{d_count, 4}, {d_sum, 8}, {d_sumsq, 8}, {d_cross, 8}};
    if ((rc = check_op_outputs("moments_rows", ops, out, d_rets, "count must be aligned to 4 bytes, sum, sumsq, cross and d_rets to 8"))) return rc;
    if ((ops & SPRINTZ_MOM_CROSS) && ref_col >= ndims) return fail(SPRINTZ_E_INVALID, "moments_rows: ref_col must be a column of the batch");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    qs.win.ops = 0;
    qs.win.row_count = (uint32_t*)out[0].p;
    qs.win.sum = (uint64_t*)out[1].p;
    qs.mom.sumsq = (uint64_t*)out[2].p;
    qs.mom.cross = (uint64_t*)out[3].p;
    qs.mom.ref = (ops & SPRINTZ_MOM_CROSS) ? ref_col : 0u;
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- extrema rows
int sprintz_mi355x_extrema_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t window_rows, uint32_t ops,
                                uint32_t flags, void* d_min, void* d_max, uint32_t* d_argmin, uint32_t* d_argmax,
                                void* d_first, void* d_last, uint32_t* d_rows, uint32_t* d_count, int64_t* d_rets,
                                void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("extrema_rows", kQueryExtrema, b, flags, d_mask, qs);
    if (rc) return rc;
    if ((rc = windowed_row_op("extrema_rows", window_rows, b, qs))) return rc;
    if (ops < 1 || ops > 255) return fail(SPRINTZ_E_INVALID, "extrema_rows: ops must be a non-empty OR of SPRINTZ_EXT_MIN / _MAX / _ARGMIN / _ARGMAX / _FIRST / _LAST / _ROWS / _COUNT");
    static_assert(SPRINTZ_EXT_MIN == 1u && SPRINTZ_EXT_MAX == 2u && SPRINTZ_EXT_ARGMIN == 4u && SPRINTZ_EXT_ARGMAX == 8u && SPRINTZ_EXT_FIRST == 16u &&
                  SPRINTZ_EXT_LAST == 32u && SPRINTZ_EXT_ROWS == 64u && SPRINTZ_EXT_COUNT == 128u && SPRINTZ_EXT_NO_ROW == kExtNoRow, "out[i] is op bit i");
    OpOutput out[8] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_argmin, 4}, {d_argmax, 4}, {d_first, elem_bytes}, {d_last, elem_bytes}, {d_rows, 4}, {d_count, 4}};
    if ((rc = check_op_outputs("extrema_rows", ops, out, nullptr, "min / max / first / last must be aligned to the element size, argmin / argmax / rows / count to 4 bytes"))) return rc;
    if ((uintptr_t)d_rets % 8) return fail(SPRINTZ_E_INVALID, "extrema_rows: d_rets must be aligned to 8 bytes");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    qs.win.ops = ops;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.row_count = (uint32_t*)out[7].p;
    qs.ext = ExtremaArgs{(uint32_t*)out[2].p, (uint32_t*)out[3].p, out[4].p, out[5].p, (uint32_t*)out[6].p};
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- segment rows
int sprintz_mi355x_segment_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t mode, const uint64_t* d_bases,
                                uint64_t capacity, uint32_t ops, uint32_t flags, void* d_min, void* d_max, uint64_t* d_sum,
                                uint32_t* d_rows, uint64_t* d_start, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("segment_rows", kQuerySegment, b, flags, d_mask, qs);
    if (rc) return rc;
    static_assert(SPRINTZ_SEG_RUNS == kSegRuns && SPRINTZ_SEG_SPLITS == kSegSplits, "the rule travels as it is given");
    if (mode != SPRINTZ_SEG_RUNS && mode != SPRINTZ_SEG_SPLITS) return fail(SPRINTZ_E_INVALID, "segment_rows: mode must be SPRINTZ_SEG_RUNS or SPRINTZ_SEG_SPLITS");
    if (ops < 1 || ops > 31) return fail(SPRINTZ_E_INVALID, "segment_rows: ops must be a non-empty OR of SPRINTZ_SEG_MIN / _MAX / _SUM / _ROWS / _START");
    if (!d_mask || !d_bases) return fail(SPRINTZ_E_INVALID, "segment_rows: null device pointer");
    static_assert(SPRINTZ_SEG_MIN == 1u && SPRINTZ_SEG_MAX == 2u && SPRINTZ_SEG_SUM == 4u && SPRINTZ_SEG_ROWS == 8u && SPRINTZ_SEG_START == 16u, "out[i] is op bit i");
    OpOutput out[5] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_sum, 8}, {d_rows, 4}, {d_start, 8}};
    if ((rc = check_op_outputs("segment_rows", ops, out, d_rets, "min / max must be aligned to the element size, rows to 4 bytes, sum, start and d_rets to 8"))) return rc;
    if ((uintptr_t)d_bases % 8) return fail(SPRINTZ_E_INVALID, "segment_rows: d_bases must be aligned to 8 bytes");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode has no struct of its own (decode_ops.h, segment rows): the rule rides where the windowed modes keep W, the places are select's
    qs.win.rows = mode;
    qs.win.count = 0;
    qs.win.ops = ops & 7u;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.sum = (uint64_t*)out[2].p;
    qs.win.row_count = (uint32_t*)out[3].p;
    qs.select = SelectArgs{d_bases, capacity, (uint64_t*)out[4].p, chunk_len / ndims};
    return decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
}

int sprintz_mi355x_segment_count(const uint8_t* d_mask, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, uint32_t mode,
                                 const int64_t* d_lens, uint32_t* d_counts, void* hip_stream)
{
    if (ndims == 0 || chunk_len == 0 || chunk_len > (1u << 30)) return fail(SPRINTZ_E_INVALID, "segment_count: ndims == 0 or chunk_len outside 1..2^30");
    if (chunk_len % ndims) return fail(SPRINTZ_E_INVALID, "segment_count: chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if (mode != SPRINTZ_SEG_RUNS && mode != SPRINTZ_SEG_SPLITS) return fail(SPRINTZ_E_INVALID, "segment_count: mode must be SPRINTZ_SEG_RUNS or SPRINTZ_SEG_SPLITS");
    if (nchunks > 0 && (!d_mask || !d_counts)) return fail(SPRINTZ_E_INVALID, "segment_count: null device pointer");
    if ((uintptr_t)d_counts % 4 || (uintptr_t)d_lens % 8) return fail(SPRINTZ_E_INVALID, "segment_count: d_counts must be aligned to 4 bytes, d_lens to 8");
    if (nchunks == 0) return 0;
    int rc = ensure_device();
    if (rc) return rc;
    if (launch_segment_count(d_mask, nchunks, chunk_len / ndims, ndims, mode, d_lens, d_counts, (hipStream_t)hip_stream) != hipSuccess)
        return fail(SPRINTZ_E_HIP, "segment_count kernel launch");
    return 0;
}

// ---------------------------------------------------------------- float rows
int sprintz_mi355x_float_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                              uint32_t chunk_len, uint16_t ndims, int out_format, const float* d_scale, const float* d_offset,
                              uint32_t flags, void* d_out, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    // (the signed bit is this operation's own flag: the shared checks see the rest)
    int rc = masked_row_op("float_rows", kQueryFloat, b, flags & ~(uint32_t)SPRINTZ_FLOAT_SIGNED, nullptr, qs);
    if (rc) return rc;
    static_assert(SPRINTZ_FLOAT_F32 == (int)kFloatF32 && SPRINTZ_FLOAT_F16 == (int)kFloatF16 && SPRINTZ_FLOAT_BF16 == (int)kFloatBF16, "the format travels as it is given");
    if (out_format != SPRINTZ_FLOAT_F32 && out_format != SPRINTZ_FLOAT_F16 && out_format != SPRINTZ_FLOAT_BF16)
        return fail(SPRINTZ_E_INVALID, "float_rows: out_format must be SPRINTZ_FLOAT_F32, SPRINTZ_FLOAT_F16 or SPRINTZ_FLOAT_BF16");
    if (!d_out) return fail(SPRINTZ_E_INVALID, "float_rows: null device pointer");
    const uint32_t mode = (uint32_t)out_format | ((flags & SPRINTZ_FLOAT_SIGNED) ? kFloatSignedBit : 0u);
    if ((uintptr_t)d_out % (uintptr_t)float_out_bytes(mode)) return fail(SPRINTZ_E_INVALID, "float_rows: d_out must be aligned to the output element size");
    if ((uintptr_t)d_scale % 4 || (uintptr_t)d_offset % 4 || (uintptr_t)d_rets % 8)
        return fail(SPRINTZ_E_INVALID, "float_rows: d_scale and d_offset must be aligned to 4 bytes, d_rets to 8");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode shares FilterArgs, as the linear filter does (decode_ops.h, float rows): lo is the scale, hi the offset, mode the format and the signed bit
    qs.rows = RowMaskArgs{};
    qs.filter.lo = d_scale;
    qs.filter.hi = d_offset;
    qs.filter.mode = mode;
    return decode_batch(b, d_out, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- rolling rows
int sprintz_mi355x_rolling_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, uint32_t window_rows, uint32_t ops, uint32_t flags,
                                void* d_min, void* d_max, int32_t* d_sum, void* d_tmp, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = unmasked_row_op("rolling_rows", b, flags);
    if (rc) return rc;
    if (window_rows < 8 || window_rows % 8) return fail_op(SPRINTZ_E_INVALID, "rolling_rows", "window_rows must be a multiple of 8, at least 8");
    if (window_rows > chunk_len / ndims) return fail_op(SPRINTZ_E_INVALID, "rolling_rows", "window_rows must not exceed the rows of a chunk, chunk_len / ndims");
    if (window_rows > roll_sum_max_window(elem_bytes)) return fail_op(SPRINTZ_E_INVALID, "rolling_rows", "window_rows x the largest element must stay below 2^31: the sum is an int32");
    if (ops < 1 || ops > 7) return fail(SPRINTZ_E_INVALID, "rolling_rows: ops must be a non-empty OR of SPRINTZ_ROLL_MIN / _MAX / _SUM");
    static_assert(SPRINTZ_ROLL_MIN == kRollMin && SPRINTZ_ROLL_MAX == kRollMax && SPRINTZ_ROLL_SUM == kRollSum, "out[i] is op bit i");
    // an output WITHOUT its op is refused too: min, max and sum are this operation's only results
    if ((d_min && !(ops & kRollMin)) || (d_max && !(ops & kRollMax)) || (d_sum && !(ops & kRollSum)))
        return fail_op(SPRINTZ_E_INVALID, "rolling_rows", "an output buffer without its op");
    OpOutput out[3] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_sum, 4}};
    if ((rc = check_op_outputs("rolling_rows", ops, out, d_rets, "min / max must be aligned to the element size, sum to 4 bytes, d_rets to 8"))) return rc;
    if (nchunks > 1 && (!d_tmp || (uintptr_t)d_tmp % 16))
        return fail_op(SPRINTZ_E_INVALID, "rolling_rows", "with more than one chunk, d_tmp must hold nchunks x the seam stride bytes, aligned to 16");
    // the rings of a workgroup's chunks must fit its LDS: the bound the planner refuses by, named here
    const uint32_t wmax = roll_shape_max_window(ndims, elem_bytes, (flags & SPRINTZ_QUERY_GENERAL_LAYOUT) != 0);
    if (window_rows > wmax) {
        const std::string what = "rolling_rows: window_rows " + std::to_string(window_rows) + " needs more LDS than a workgroup has for this shape's history rings: the largest window_rows allowed is " +
                                 std::to_string(wmax);
        return fail(SPRINTZ_E_UNSUPPORTED, what.c_str());
    }
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode shares structs that exist (decode_ops.h, rolling rows): W, the ops and the outputs in WindowArgs, the seam scratch in LinearArgs::tmp
    QuerySpec qs = row_query(kQueryRolling, flags);
    qs.win.rows = window_rows;
    qs.win.ops = ops;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.sum = (uint64_t*)out[2].p;
    qs.lin.tmp = nchunks > 1 ? d_tmp : nullptr;
    rc = decode_batch(b, nullptr, d_rets, (hipStream_t)hip_stream, qs);
    if (rc || nchunks < 2) return rc;
    // the seam pass, behind the decode on the same stream
    DecodeArgs a{};
    a.nchunks = nchunks;
    a.chunk_len = chunk_len;
    a.D = ndims;
    a.win = qs.win;
    a.lin = qs.lin;
    if (launch_rolling_seam(elem_bytes, a, (hipStream_t)hip_stream) != hipSuccess) return fail(SPRINTZ_E_HIP, "rolling_rows seam kernel launch");
    return 0;
}

// ---------------------------------------------------------------- project rows
int sprintz_mi355x_project_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint32_t ndims, const int32_t* d_slots, uint32_t ncolumns, int format,
                                const float* d_scale, const float* d_offset, uint32_t flags, void* d_out, int64_t* d_rets, void* hip_stream)
{
    if (ndims > 0xffffu) return fail(SPRINTZ_E_UNSUPPORTED, "project_rows: more than 512 columns");
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, (uint16_t)ndims};
    // (the signed bit is float rows' flag: the shared checks see the rest)
    int rc = unmasked_row_op("project_rows", b, flags & ~(uint32_t)SPRINTZ_FLOAT_SIGNED);
    if (rc) return rc;
    if (ncolumns == 0) return fail_op(SPRINTZ_E_INVALID, "project_rows", "ncolumns == 0: an output row has at least one column");
    if (ncolumns > ndims) return fail_op(SPRINTZ_E_INVALID, "project_rows", "ncolumns above ndims: the columns of the output are distinct columns of the batch");
    static_assert(SPRINTZ_PROJECT_F32 == 1 + SPRINTZ_FLOAT_F32 && SPRINTZ_PROJECT_F16 == 1 + SPRINTZ_FLOAT_F16 && SPRINTZ_PROJECT_BF16 == 1 + SPRINTZ_FLOAT_BF16,
                  "a float format travels as float rows' number");
    if (format != SPRINTZ_PROJECT_RAW && format != SPRINTZ_PROJECT_F32 && format != SPRINTZ_PROJECT_F16 && format != SPRINTZ_PROJECT_BF16)
        return fail(SPRINTZ_E_INVALID, "project_rows: format must be SPRINTZ_PROJECT_RAW, SPRINTZ_PROJECT_F32, SPRINTZ_PROJECT_F16 or SPRINTZ_PROJECT_BF16");
    const bool raw = format == SPRINTZ_PROJECT_RAW;
    if (raw && (d_scale || d_offset || (flags & SPRINTZ_FLOAT_SIGNED)))
        return fail_op(SPRINTZ_E_INVALID, "project_rows", "d_scale, d_offset and SPRINTZ_FLOAT_SIGNED go with a float format only");
    if (!d_slots || !d_out) return fail(SPRINTZ_E_INVALID, "project_rows: null device pointer");
    const uint32_t mode = raw ? kProjectRawBit : (uint32_t)(format - 1) | ((flags & SPRINTZ_FLOAT_SIGNED) ? kFloatSignedBit : 0u);
    if ((uintptr_t)d_out % (uintptr_t)project_out_bytes(mode, elem_bytes)) return fail(SPRINTZ_E_INVALID, "project_rows: d_out must be aligned to the output element size");
    if ((uintptr_t)d_slots % 4 || (uintptr_t)d_scale % 4 || (uintptr_t)d_offset % 4 || (uintptr_t)d_rets % 8)
        return fail(SPRINTZ_E_INVALID, "project_rows: d_slots, d_scale and d_offset must be aligned to 4 bytes, d_rets to 8");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode shares FilterArgs, as float rows do (decode_ops.h, project rows): lo the scale, hi the offset, mode the format; mask the slot table, mask_stride K
    QuerySpec qs = row_query(kQueryProject, flags);
    qs.filter.lo = d_scale;
    qs.filter.hi = d_offset;
    qs.filter.mode = mode;
    qs.filter.mask = (uint8_t*)const_cast<int32_t*>(d_slots);
    qs.filter.mask_stride = ncolumns;
    return decode_batch(b, d_out, d_rets, (hipStream_t)hip_stream, qs);
}

// ---------------------------------------------------------------- derive rows
uint64_t sprintz_mi355x_derive_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims)
{
    return sprintz_mi355x_filter_linear_tmp_bytes(elem_bytes, nchunks, ndims);      // the linear filter's scratch, as it is (decode_ops.h: LinearSlot)
}

int sprintz_mi355x_derive_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, uint32_t nforms, const int32_t* d_weights, const int32_t* d_lag_weights,
                               const int32_t* d_bias, int format, const float* d_scale, const float* d_offset, const void* d_prev,
                               uint32_t flags, void* d_tmp, void* d_out, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = unmasked_row_op("derive_rows", b, flags);
    if (rc) return rc;
    if (nforms < 1 || nforms > kDeriveMaxForms) return fail_op(SPRINTZ_E_INVALID, "derive_rows", "nforms must be in 1 .. 16");
    static_assert(SPRINTZ_DERIVE_F32 == 1 + SPRINTZ_FLOAT_F32 && SPRINTZ_DERIVE_F16 == 1 + SPRINTZ_FLOAT_F16 && SPRINTZ_DERIVE_BF16 == 1 + SPRINTZ_FLOAT_BF16,
                  "a float format travels as float rows' number");
    if (format != SPRINTZ_DERIVE_I32 && format != SPRINTZ_DERIVE_F32 && format != SPRINTZ_DERIVE_F16 && format != SPRINTZ_DERIVE_BF16)
        return fail(SPRINTZ_E_INVALID, "derive_rows: format must be SPRINTZ_DERIVE_I32, SPRINTZ_DERIVE_F32, SPRINTZ_DERIVE_F16 or SPRINTZ_DERIVE_BF16");
    const bool i32 = format == SPRINTZ_DERIVE_I32;
    if (i32 && (d_scale || d_offset)) return fail_op(SPRINTZ_E_INVALID, "derive_rows", "d_scale and d_offset go with a float format only");
    if (!d_weights || !d_out) return fail(SPRINTZ_E_INVALID, "derive_rows: null device pointer");
    const uint32_t mode = i32 ? kDeriveI32Bit : (uint32_t)(format - 1);
    if ((uintptr_t)d_out % (uintptr_t)derive_out_bytes(mode)) return fail(SPRINTZ_E_INVALID, "derive_rows: d_out must be aligned to the output element size");
    if ((uintptr_t)d_weights % 4 || (uintptr_t)d_lag_weights % 4 || (uintptr_t)d_bias % 4 || (uintptr_t)d_scale % 4 || (uintptr_t)d_offset % 4 ||
        (uintptr_t)d_prev % (uintptr_t)elem_bytes || (uintptr_t)d_rets % 8)
        return fail(SPRINTZ_E_INVALID, "derive_rows: d_weights, d_lag_weights, d_bias, d_scale and d_offset must be aligned to 4 bytes, d_prev to the element size, d_rets to 8");
    if (d_lag_weights && (!d_tmp || (uintptr_t)d_tmp % 8))
        return fail(SPRINTZ_E_INVALID, "derive_rows: with d_lag_weights, d_tmp must hold sprintz_mi355x_derive_rows_tmp_bytes bytes, aligned to 8");
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode shares structs that exist (decode_ops.h, derive rows): the weight tables and the seam scratch in LinearArgs; scale, offset, format,
    // biases, the `prev` row and K in FilterArgs
    QuerySpec qs = row_query(kQueryDerive, flags);
    qs.lin = LinearArgs{d_weights, d_lag_weights, d_lag_weights ? d_tmp : nullptr, 0, 0, 0, 0u};
    qs.filter.lo = d_scale;
    qs.filter.hi = d_offset;
    qs.filter.mode = mode;
    qs.filter.mask = (uint8_t*)const_cast<int32_t*>(d_bias);
    qs.filter.counts = d_lag_weights ? (uint32_t*)const_cast<void*>(d_prev) : nullptr;
    qs.filter.mask_stride = nforms;
    rc = decode_batch(b, d_out, d_rets, (hipStream_t)hip_stream, qs);
    if (rc || !d_lag_weights || (nchunks < 2 && !d_prev)) return rc;
    // the seam pass, behind the decode on the same stream: row 0 of every chunk behind the first -- and of the first, with d_prev -- takes its true predecessor
    DecodeArgs a{};
    a.nchunks = nchunks;
    a.chunk_len = chunk_len;
    a.D = ndims;
    a.out = d_out;
    a.filter = qs.filter;
    a.lin = qs.lin;
    if (launch_derive_seam(elem_bytes, a, (hipStream_t)hip_stream) != hipSuccess) return fail(SPRINTZ_E_HIP, "derive_rows seam kernel launch");
    return 0;
}

// ---------------------------------------------------------------- FIR rows
uint64_t sprintz_mi355x_fir_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims, uint32_t ntaps)
{
    if ((elem_bytes != 1 && elem_bytes != 2) || ndims == 0 || ntaps < 2 || ntaps > kFirMaxTaps) return 0;
    return nchunks * fir_tmp_stride(ntaps, ndims, elem_bytes);
}

int sprintz_mi355x_fir_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                            uint32_t chunk_len, uint16_t ndims, uint32_t ntaps, const int32_t* d_taps, const int32_t* d_bias, int format,
                            const float* d_scale, const float* d_offset, const void* d_prev, uint32_t flags, void* d_tmp, void* d_out,
                            int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = unmasked_row_op("fir_rows", b, flags);
    if (rc) return rc;
    if (ntaps < 1 || ntaps > kFirMaxTaps) return fail_op(SPRINTZ_E_INVALID, "fir_rows", "ntaps must be in 1 .. 256");
    if (ntaps - 1u > chunk_len / ndims) return fail_op(SPRINTZ_E_INVALID, "fir_rows", "ntaps - 1 must not exceed the rows of a chunk, chunk_len / ndims");
    if (format != SPRINTZ_DERIVE_I32 && format != SPRINTZ_DERIVE_F32 && format != SPRINTZ_DERIVE_F16 && format != SPRINTZ_DERIVE_BF16)
        return fail(SPRINTZ_E_INVALID, "fir_rows: format must be SPRINTZ_DERIVE_I32, SPRINTZ_DERIVE_F32, SPRINTZ_DERIVE_F16 or SPRINTZ_DERIVE_BF16");
    const bool i32 = format == SPRINTZ_DERIVE_I32;
    if (i32 && (d_scale || d_offset)) return fail_op(SPRINTZ_E_INVALID, "fir_rows", "d_scale and d_offset go with a float format only");
    if (!d_taps || !d_out) return fail(SPRINTZ_E_INVALID, "fir_rows: null device pointer");
    const uint32_t mode = i32 ? kDeriveI32Bit : (uint32_t)(format - 1);
    if ((uintptr_t)d_out % (uintptr_t)derive_out_bytes(mode)) return fail(SPRINTZ_E_INVALID, "fir_rows: d_out must be aligned to the output element size");
    if ((uintptr_t)d_taps % 4 || (uintptr_t)d_bias % 4 || (uintptr_t)d_scale % 4 || (uintptr_t)d_offset % 4 ||
        (ntaps > 1 && (uintptr_t)d_prev % (uintptr_t)elem_bytes) || (uintptr_t)d_rets % 8)      // (one tap: d_prev is ignored, whatever it is)
        return fail(SPRINTZ_E_INVALID, "fir_rows: d_taps, d_bias, d_scale and d_offset must be aligned to 4 bytes, d_prev to the element size, d_rets to 8");
    if (ntaps > 1 && (!d_tmp || (uintptr_t)d_tmp % 16))
        return fail(SPRINTZ_E_INVALID, "fir_rows: with ntaps > 1, d_tmp must hold sprintz_mi355x_fir_rows_tmp_bytes bytes, aligned to 16");
    // the rings of a workgroup's chunks must fit its LDS: the bound the planner refuses by, named here
    const uint32_t tmax = fir_shape_max_taps(ndims, elem_bytes, (flags & SPRINTZ_QUERY_GENERAL_LAYOUT) != 0);
    if (ntaps > tmax) {
        const std::string what = "fir_rows: ntaps " + std::to_string(ntaps) + " needs more LDS than a workgroup has for this shape's history rings: the largest ntaps allowed is " +
                                 std::to_string(tmax);
        return fail(SPRINTZ_E_UNSUPPORTED, what.c_str());
    }
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    // the mode shares structs that exist (decode_ops.h, FIR rows): T and the history's rows in WindowArgs; the taps, the biases and the seam scratch in
    // LinearArgs; scale, offset, format and the `prev` rows in FilterArgs
    QuerySpec qs = row_query(kQueryFir, flags);
    qs.win.rows = fir_history_rows(ntaps);
    qs.win.count = ntaps;
    qs.lin = LinearArgs{d_taps, d_bias, ntaps > 1 ? d_tmp : nullptr, 0, 0, 0, 0u};
    qs.filter.lo = d_scale;
    qs.filter.hi = d_offset;
    qs.filter.mode = mode;
    qs.filter.counts = ntaps > 1 ? (uint32_t*)const_cast<void*>(d_prev) : nullptr;
    rc = decode_batch(b, d_out, d_rets, (hipStream_t)hip_stream, qs);
    if (rc || ntaps < 2) return rc;
    // the seam pass, behind the decode on the same stream: the first ntaps - 1 rows of every chunk, computed again from raw rows
    DecodeArgs a{};
    a.nchunks = nchunks;
    a.chunk_len = chunk_len;
    a.D = ndims;
    a.out = d_out;
    a.win = qs.win;
    a.filter = qs.filter;
    a.lin = qs.lin;
    if (launch_fir_seam(elem_bytes, a, (hipStream_t)hip_stream) != hipSuccess) return fail(SPRINTZ_E_HIP, "fir_rows seam kernel launch");
    return 0;
}

// ---------------------------------------------------------------- cumulative rows
size_t sprintz_mi355x_cumulative_tmp_bytes(uint64_t nchunks, uint16_t ndims)
{
    return nchunks > 1 ? (size_t)cum_tmp_layout(nchunks, ndims ? ndims : 1).bytes : 0;
}

int sprintz_mi355x_cumulative_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                   uint32_t chunk_len, uint16_t ndims, uint32_t ops, int sum_bytes, uint32_t flags,
                                   void* d_min, void* d_max, void* d_sum, const uint64_t* d_carry_in, uint64_t* d_carry_out,
                                   void* d_tmp, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    const hipStream_t st = (hipStream_t)hip_stream;
    int rc = unmasked_row_op("cumulative_rows", b, flags);
    if (rc) return rc;
    if (ops < 1 || ops > 7) return fail(SPRINTZ_E_INVALID, "cumulative_rows: ops must be a non-empty OR of SPRINTZ_CUM_MIN / _MAX / _SUM");
    static_assert(SPRINTZ_CUM_MIN == kCumMin && SPRINTZ_CUM_MAX == kCumMax && SPRINTZ_CUM_SUM == kCumSum, "out[i] is op bit i");
    static_assert(SPRINTZ_CUM_MIN == SPRINTZ_QUERY_WIN_MIN && SPRINTZ_CUM_MAX == SPRINTZ_QUERY_WIN_MAX && SPRINTZ_CUM_SUM == SPRINTZ_QUERY_WIN_SUM,
                  "the totals pass takes the ops as they are");
    // an output WITHOUT its op is refused too: min, max and sum are this operation's only results
    if ((d_min && !(ops & kCumMin)) || (d_max && !(ops & kCumMax)) || (d_sum && !(ops & kCumSum)))
        return fail_op(SPRINTZ_E_INVALID, "cumulative_rows", "an output buffer without its op");
    if (sum_bytes != 4 && sum_bytes != 8) return fail(SPRINTZ_E_INVALID, "cumulative_rows: sum_bytes must be 4 (int32, the low half) or 8 (int64)");
    OpOutput out[3] = {{d_min, elem_bytes}, {d_max, elem_bytes}, {d_sum, sum_bytes}};
    if ((rc = check_op_outputs("cumulative_rows", ops, out, d_rets, "min / max must be aligned to the element size, sum to sum_bytes, d_rets to 8"))) return rc;
    if ((uintptr_t)d_carry_in % 8 || (uintptr_t)d_carry_out % 8) return fail(SPRINTZ_E_INVALID, "cumulative_rows: d_carry_in and d_carry_out must be aligned to 8 bytes");
    if ((uintptr_t)d_tmp % 16) return fail(SPRINTZ_E_INVALID, "cumulative_rows: d_tmp must be aligned to 16 bytes");
    if (nchunks > 1 && !d_tmp)
        return fail_op(SPRINTZ_E_INVALID, "cumulative_rows", "with more than one chunk, d_tmp must hold sprintz_mi355x_cumulative_tmp_bytes(nchunks, ndims) bytes");
    if (nchunks == 0 && !d_carry_out) return 0;
    if ((rc = ensure_device())) return rc;
    if (nchunks == 0) {                                     // nothing to decode: the seeds are the state behind the batch (the scan over no chunk)
        if (launch_cumulative_scan(elem_bytes, 0, ndims, ops, nullptr, d_carry_in, d_carry_out, st) != hipSuccess) return fail(SPRINTZ_E_HIP, "cumulative_rows scan kernel launch");
        return 0;
    }
    // the mode shares structs that exist (decode_ops.h, cumulative rows): the ops, sum_bytes and the outputs in WindowArgs, the chunks' entering
    // states in LinearArgs::tmp
    QuerySpec qs = row_query(kQueryCumulative, flags);
    qs.win.ops = ops;
    qs.win.count = (uint32_t)sum_bytes;
    qs.win.min = out[0].p;
    qs.win.max = out[1].p;
    qs.win.sum = (uint64_t*)out[2].p;
    if (nchunks == 1) {
        // one chunk enters with the seeds themselves and leaves its state to carry_out: no totals, no scan, and no scratch
        qs.lin.tmp = const_cast<uint64_t*>(d_carry_in);
        qs.lin.w = (const int32_t*)d_carry_out;
        return decode_batch(b, nullptr, d_rets, st, qs);
    }
    // 1. the totals: every chunk's per-column min / max / sum and its return value, the windowed query with one window a chunk
    const CumTmp lay = cum_tmp_layout(nchunks, ndims);
    uint8_t* const tmp = (uint8_t*)d_tmp;
    const uint32_t rows = chunk_len / ndims;
    QuerySpec tq = row_query(kQueryWindow, flags);
    tq.win.rows = rows < 8 ? 8u : (rows + 7u) & ~7u;
    tq.win.count = 1;
    tq.win.ops = ops;
    tq.win.min = (ops & kCumMin) ? tmp + lay.min : nullptr;
    tq.win.max = (ops & kCumMax) ? tmp + lay.max : nullptr;
    tq.win.sum = (ops & kCumSum) ? (uint64_t*)(tmp + lay.sum) : nullptr;
    if ((rc = decode_batch(b, nullptr, (int64_t*)(tmp + lay.rets), st, tq))) return rc;
    // 2. the scan: each chunk's entering state, and the state behind the last one
    if (launch_cumulative_scan(elem_bytes, nchunks, ndims, ops, tmp, d_carry_in, d_carry_out, st) != hipSuccess) return fail(SPRINTZ_E_HIP, "cumulative_rows scan kernel launch");
    // 3. the decode
    qs.lin.tmp = tmp + lay.state;
    return decode_batch(b, nullptr, d_rets, st, qs);
}

// ---------------------------------------------------------------- histogram rows
int sprintz_mi355x_histogram_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                  uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, const void* d_lo, uint32_t shift, uint32_t nbins,
                                  uint64_t hist_chunks, uint32_t flags, uint64_t* d_hist, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("histogram_rows", kQueryHistogram, b, flags, d_mask, qs);
    if (rc) return rc;
    if ((rc = binned_row_op("histogram_rows", elem_bytes, shift, nbins))) return rc;
    if (!d_hist) return fail(SPRINTZ_E_INVALID, "histogram_rows: null device pointer");
    if ((uintptr_t)d_hist % 8 || (uintptr_t)d_rets % 8) return fail(SPRINTZ_E_INVALID, "histogram_rows: d_hist and d_rets must be aligned to 8 bytes");
    if (d_lo && (uintptr_t)d_lo % (uintptr_t)elem_bytes) return fail(SPRINTZ_E_INVALID, "histogram_rows: d_lo must be aligned to the element size");
    if ((uint64_t)ndims * nbins > SPRINTZ_HIST_MAX_COUNTERS)
        return fail(SPRINTZ_E_UNSUPPORTED, "histogram_rows: ndims x nbins above SPRINTZ_HIST_MAX_COUNTERS: split the bins with d_lo");
    uint64_t ngroups;
    if ((rc = binned_tables(nchunks, hist_chunks, ndims, nbins, "histogram_rows: too many histograms for one call (ngroups x ndims x nbins above 2^40 entries)", &ngroups)))
        return rc;
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    qs.table = BinTableArgs{hist_chunks, shift, nbins, 0, 0, (uint32_t)ndims * nbins};
    qs.table_row_max = 1;
    qs.hist = HistogramArgs{d_lo, d_hist};
    return binned_launch(b, d_rets, (hipStream_t)hip_stream, qs, [&](hipStream_t st) {
        HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)(ngroups * ndims * nbins * 8), st));
        return 0;
    });
}

// ---------------------------------------------------------------- group-by rows
int sprintz_mi355x_groupby_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t key_col, uint32_t key_lo, uint32_t shift,
                                uint32_t nbins, uint64_t table_chunks, uint32_t ops, uint32_t flags, uint64_t* d_count, uint64_t* d_sum,
                                int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    QuerySpec qs;
    int rc = masked_row_op("groupby_rows", kQueryGroupBy, b, flags, d_mask, qs);
    if (rc) return rc;
    if (key_col >= ndims) return fail(SPRINTZ_E_INVALID, "groupby_rows: key_col must be a column of the batch");
    if (key_lo >= (1u << (8 * elem_bytes))) return fail(SPRINTZ_E_INVALID, "groupby_rows: key_lo must be below 2^W");
    if ((rc = binned_row_op("groupby_rows", elem_bytes, shift, nbins))) return rc;
    if (ops == 0 || (ops & ~(SPRINTZ_GBY_COUNT | SPRINTZ_GBY_SUM))) return fail(SPRINTZ_E_INVALID, "groupby_rows: ops must be a non-empty OR of SPRINTZ_GBY_COUNT / _SUM");
    static_assert(SPRINTZ_GBY_COUNT == 1u && SPRINTZ_GBY_SUM == 2u, "out[i] is op bit i");
    OpOutput out[2] = {{d_count, 8}, {d_sum, 8}};
    if ((rc = check_op_outputs("groupby_rows", ops, out, d_rets, "d_count, d_sum and d_rets must be aligned to 8 bytes"))) return rc;
    if ((uint64_t)nbins * ((uint64_t)ndims + 1) > SPRINTZ_GBY_MAX_COUNTERS)
        return fail(SPRINTZ_E_UNSUPPORTED, "groupby_rows: nbins x (ndims + 1) above SPRINTZ_GBY_MAX_COUNTERS: split the bins with key_lo");
    uint64_t ntables;
    if ((rc = binned_tables(nchunks, table_chunks, ndims, nbins, "groupby_rows: too many tables for one call (ntables x nbins x ndims above 2^40 entries)", &ntables)))
        return rc;
    if (nchunks == 0) return 0;
    if ((rc = ensure_device())) return rc;
    qs.table = BinTableArgs{table_chunks, shift, nbins, 0, 0, nbins * ((uint32_t)ndims + 1u)};
    qs.table_row_max = (1u << (8 * elem_bytes)) - 1u;
    qs.gby = GroupByArgs{(uint64_t*)out[0].p, (uint64_t*)out[1].p, key_col, key_lo};
    return binned_launch(b, d_rets, (hipStream_t)hip_stream, qs, [&](hipStream_t st) {
        if (qs.gby.count) HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)(ntables * nbins * 8), st));
        if (qs.gby.sum) HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)(ntables * nbins * ndims * 8), st));
        return 0;
    });
}

// ---------------------------------------------------------------- gather rows
int sprintz_mi355x_gather_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const uint64_t* d_starts, uint64_t nranges, uint32_t rows,
                               void* d_out, int64_t* d_rets, void* hip_stream)
{
    const Batch b{codec, elem_bytes, d_comp, d_offsets, nchunks, chunk_len, ndims};
    int rc = check_common(codec, elem_bytes, ndims);
    if (rc) return rc;
    if ((rc = check_row_op(b, 0, "more than 512 columns: no gather", "gather_rows: the RLE codecs (delta, xff) only"))) return rc;
    if (chunk_len % ndims) return fail(SPRINTZ_E_INVALID, "gather_rows: chunk_len must be a multiple of ndims (rows must not straddle chunks)");
    if (rows == 0) return fail(SPRINTZ_E_INVALID, "gather_rows: rows == 0");
    if (!d_out) return fail(SPRINTZ_E_INVALID, "null device pointer");
    if (nranges > 0 && !d_starts) return fail(SPRINTZ_E_INVALID, "gather_rows: ranges without their starts");
    if ((uintptr_t)d_out % (uintptr_t)elem_bytes) return fail(SPRINTZ_E_INVALID, "gather_rows: d_out must be aligned to the element size");
    if ((uintptr_t)d_starts % 8 || (uintptr_t)d_rets % 8) return fail(SPRINTZ_E_INVALID, "gather_rows: d_starts and d_rets must be aligned to 8 bytes");
    const int D = ndims, esz = elem_bytes;
    const uint32_t R = chunk_len / ndims;
    const uint64_t P = gather_pieces(rows, R);
    if (nranges > (1ull << 40) || nranges * P > (1ull << 40)) return fail(SPRINTZ_E_INVALID, "gather_rows: too many pieces for one launch");
    if ((rc = ensure_device())) return rc;
    if (nranges == 0) return 0;
    hipStream_t st = (hipStream_t)hip_stream;

    Shape s;
    s.codec = codec; s.esz = esz; s.D = D; s.nchunks = nchunks; s.chunk_len = chunk_len; s.nranges = nranges; s.rows = rows; s.out_lo = low4(d_out);
    const Plan p = plan_gather(s, snapshot());
    QuerySpec qs;
    qs.q = kQueryGather;
    qs.gather = GatherArgs{d_starts, nranges, rows, R, (uint32_t)P};
    if (d_rets) {                                          // (in front of the plan's verdict: a refused call leaves its entries filled, too)
        hipLaunchKernelGGL(gather_rets_fill, dim3((unsigned)((nranges + 255) / 256)), dim3(256), 0, st, d_rets, nranges, (int64_t)rows);
        HIP_TRY(hipGetLastError());
    }
    return decode_launch(p, b, d_out, d_rets, st, qs);
}

int sprintz_mi355x_query_reduce(int op, const uint64_t* d_partials, uint64_t nchunks, uint16_t ndims, uint64_t* d_result,
                                void* hip_stream)
{
    if (op != 1 && op != 2) return fail(SPRINTZ_E_INVALID, "op must be 1 (max) or 2 (sum)");
    if (!d_partials || !d_result || ndims == 0) return fail(SPRINTZ_E_INVALID, "null device pointer");
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(d_result, 0, (size_t)ndims * 8, st));
    if (nchunks == 0) return 0;
    const uint32_t RB = ndims >= 256 ? 1u : 256u / ndims;
    uint64_t blocks = (nchunks + RB - 1) / RB;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(query_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_partials, nchunks, (uint32_t)ndims, op,
                       (unsigned long long*)d_result);
    return hipGetLastError() == hipSuccess ? 0 : fail(SPRINTZ_E_HIP, "query_reduce launch");
}

}  // extern "C"
