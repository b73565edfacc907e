// entry.h -- what the units of the entry layer share, host only: the error sink and the process-wide facts (api.hip), the
// descriptors a call is handed down by, and the glue between plan.h and the launchers.  api.hip holds the batched calls,
// host_call.hip the single calls on host pointers, row_ops.hip the row operations; huf*.hip, transforms.hip, zone.hip and
// online.hip take the error sink, the device probe, the size scan and the pooled scratch from here.
#pragma once

#include "../../include/sprintz_mi355x.h"

#include <hip/hip_runtime.h>
#include <atomic>

#include "launch.h"
#include "dispatch.h"
#include "plan.h"

namespace sprintz {

// records `what` (and e's text, if any) as this thread's last error (sprintz_mi355x_last_error) and returns `code`: every
// failing return of every translation unit goes through it, so the message is never stale
int fail(int code, const char* what, hipError_t e = hipSuccess);
// a refusal in the words several operations share, with the operation's name in front (op == null: as they are)
int fail_op(int code, const char* op, const char* what);

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t e_ = (expr);                                               \
        if (e_ != hipSuccess) return ::sprintz::fail(SPRINTZ_E_HIP, #expr, e_); \
    } while (0)

bool have_device();      // probed once per process
int ensure_device();     // ... and its refusal
Knobs snapshot();        // the dispatch options as ONE exported call sees them (plan.h)
int check_common(int codec, int esz, uint16_t ndims);
int check_batch_tail(uint64_t total_len, uint32_t chunk_len, uint16_t ndims);

// exclusive scan of (aligned) u32 sizes into u64 offsets[n+1]; tmp = sprintz_mi355x_compact_tmp_bytes(n)
hipError_t launch_size_scan(const uint32_t* d_sizes, uint64_t n, uint32_t align, uint64_t* d_offsets, void* d_tmp, hipStream_t st);

// the calling thread's pooled scratch for host-pointer entry points (host_call.hip: acquire_scratch): buffers only grow, the
// stream is private and non-blocking; valid until the thread's next host_scratch() call
struct HostScratch { hipStream_t stream; uint8_t* dev; uint8_t* pin; };
int host_scratch(size_t dev_bytes, size_t pin_bytes, HostScratch* out);

std::atomic<long long>& huf0_sync_chunks(); // huf0.hip: batch size up to which the stream stage runs as a wave per chunk with self-synchronising decoders (huf0_sync.h)
std::atomic<long long>& huf0_big_batch(); // huf0.hip: batch size from which the one-table stream kernel runs as workgroups of HUF0_BIG_WG (2) waves

inline unsigned low4(const void* p) { return (unsigned)((uintptr_t)p & 15u); }

// a compressed batch, as every decoding entry point is handed it
struct Batch {
    int codec, esz;
    const void* comp;
    const uint64_t* offsets;
    uint64_t nchunks;
    uint32_t chunk_len;
    uint16_t ndims;
};
// what an encoding entry point is handed: the source, the slots, the sizes / return values
struct EncodeBatch {
    int codec, esz;
    const void* src;
    uint64_t total_len;
    uint32_t chunk_len;
    uint16_t ndims;
    void* slots;
    size_t slot_stride;
    uint32_t* sizes;
    int64_t* rets;
    int write_size = 1;
    uint64_t col_stride = 0;    // != 0: column-major source
    int general = 0;            // 1: general row-major layout for every ndims
    // a float source (quant.h): src holds float32 / float16 / bfloat16, quantised with the columns' inverse scales and offsets
    // (null: all 1 / all 0) under q_mode -- the format, kFloatSignedBit, kQuantFloorBit
    bool fsrc = false;
    const float* q_inv = nullptr;
    const float* q_off = nullptr;
    uint32_t q_mode = 0;
};
// where the encode launch builds the dense container itself (compact_tail.h; Plan::fused)
struct DenseRequest { void* d_dense; uint64_t* d_offsets; void* d_tmp; };

// a single call served straight from the caller thread's mapped host buffer by ONE launch of a workgroup-per-chunk kernel
// (decode_lat.h / encode_lat.h): no staging kernel in front, no runtime wait behind -- the kernel's last store is the
// call's ticket into a mapped host word
struct HostCall {
    uint64_t off0 = 0, off1 = 0;   // decode: the stream is comp[off0, off1)
    uint64_t* flag = nullptr;      // device view of the word
    uint64_t ticket = 0;
};

// query-on-compressed options of one decode launch (the decoders' Q template parameter; decode_ops.h)
struct QuerySpec {
    int q = kQueryOff;          // kQueryOff .. kQueryFir (geom.h)
    int qop = 0;                // 1 max, 2 sum
    uint64_t* qres = nullptr;   // [nchunks][ndims]
    // the mode's own arguments, as the kernels take them (decode_ops.h)
    WindowArgs win{};           // kQueryWindow
    GatherArgs gather{};        // kQueryGather
    FilterArgs filter{};        // kQueryFilter
    SelectArgs select{};        // kQuerySelect (with rows)
    RowMaskArgs rows{};         // kQuerySelect, kQueryAggregate (with win), and the three below
    BinTableArgs table{};       // kQueryHistogram, kQueryGroupBy (table_off and wg_chunks come from the plan)
    uint32_t table_row_max = 0; // ... the most one row can add to an entry of the table (plan.h: Shape::table_row_max)
    HistogramArgs hist{};       // kQueryHistogram
    MomentArgs mom{};           // kQueryMoments (with win)
    GroupByArgs gby{};          // kQueryGroupBy
    ExtremaArgs ext{};          // kQueryExtrema (with win and rows)
    LinearArgs lin{};           // kQueryLinear (with filter: the mask, the counts and the mask's stride)
    // (kQuerySegment has no struct of its own: win, select and rows carry it -- decode_ops.h, segment rows; kQueryFloat rides in filter: lo the scale, hi the offset, mode the format;
    //  kQueryRolling in win -- W, the ops, the outputs -- and lin.tmp, the seam scratch: decode_ops.h, rolling rows; kQueryProject in filter, as
    //  kQueryFloat does, with mask the slot table and mask_stride K: decode_ops.h, project rows;
    //  kQueryCumulative in win -- the ops, sum_bytes in count, the outputs -- lin.tmp, the chunks' entering states, and lin.w, carry_out: decode_ops.h, cumulative rows;
    //  kQueryDerive in lin -- the [K][D] weight tables and the seam scratch -- and filter: lo the scale, hi the offset, mode the format, mask the biases,
    //  counts the `prev` row, mask_stride K: decode_ops.h, derive rows;
    //  kQueryFir in win -- T in count, the history's rows in rows -- lin -- w the taps, lag the biases, tmp the seam scratch -- and filter: lo the scale, hi the
    //  offset, mode the format, counts the `prev` rows: decode_ops.h, FIR rows)
    int general = 0;            // 1: general row-major layout for every ndims (the reference's *_rowmajor_*_rle_* family)
    uint64_t col_stride = 0;    // != 0: column-major destination (DecodeArgs::col_stride)
    const HostCall* hc = nullptr;
    // the header-less framing of sprintz_mi355x_decompress_noheader: decompress_host (host_call.hip) alone sets it
    int noheader = 0;
    uint32_t nh_ngroups = 0, nh_remaining = 0;
};

// plan.h's view of a call; the launch of what it planned (the arguments from the plan, one switch on the family, the
// counter); and both at once, with the options of `k` -- or, without, of this moment
Shape decode_shape(const Batch& b, const void* d_out, const QuerySpec& qs);
int decode_launch(const Plan& p, const Batch& b, void* d_out, int64_t* d_rets, hipStream_t st, const QuerySpec& qs);
int decode_batch(const Knobs& k, const Batch& b, void* d_out, int64_t* d_rets, hipStream_t st, const QuerySpec& qs = QuerySpec{});
inline int decode_batch(const Batch& b, void* d_out, int64_t* d_rets, hipStream_t st, const QuerySpec& qs = QuerySpec{})
{
    return decode_batch(snapshot(), b, d_out, d_rets, st, qs);
}
// the same for an encode; `dense` is read only where the plan says the encoder builds the container.  encode_batch: slots only
Shape encode_shape(const EncodeBatch& j, bool dense, bool host_call);
int encode_launch(const Plan& p, const EncodeBatch& j, hipStream_t st, const DenseRequest* dense = nullptr, const HostCall* hc = nullptr);
int encode_batch(const Knobs& k, const EncodeBatch& j, hipStream_t st);

}  // namespace sprintz
