// plan.h -- which kernel serves a call, and with which launch geometry: pure functions of a shape, the dispatch options and a few
// address low bits.  No HIP call, no pointer, neither process() nor the environment: api.hip snapshots the options ONCE per exported
// call (Knobs), plans, and launches what the plan says -- nothing is decided a second time, so an option that changes while a call runs
// cannot send it to two kernels.  Plain C++17 (geom.h + the constants of sprintz_mi355x.h): the CPU tests build it with a host compiler
// and replay the GPU tier's edge table through it (tests/plan_probe.cpp, tests/test_plan_cpu.py).
//
// Every predicate keeps the terms and the ORDER it had at the launch sites, the ones that never decide included: tests/dispatch_cases.py
// pins both sides of every edge, and the measured-and-dropped notes next to the branches say why the thresholds are what they are.
#pragma once

#include "../../include/sprintz_mi355x.h"
#include "geom.h"

namespace sprintz {

// sprintz_mi355x_dispatch_name: a family's short name, by SPRINTZ_KF_* number
constexpr const char* kFamilyNames[] = {"dec_big", "dec_any", "dec_verbatim", "dec_lat", "dec_row", "dec_blk", "dec_fast", "dec_uni", "dec_generic",
                                        "gather_fast", "gather_generic",
                                        "enc_big", "enc_any", "enc_lat", "enc_blk", "enc_blk_uni", "enc_pair", "enc_fast", "enc_wide", "enc_split", "enc_uni", "enc_generic",
                                        "dense_fused", "dense_verbatim", "dense_compact",
                                        "tr_chain", "tr_wave", "tr_levels", "on_chain", "on_three", "huf0_big", "huf0_sync", "huf0_default"};
static_assert(sizeof(kFamilyNames) / sizeof(kFamilyNames[0]) == SPRINTZ_KF_COUNT, "a name per SPRINTZ_KF_* family");

// the dispatch options, as one call sees them (api.hip: snapshot())
struct Knobs {
    int no_fast = 0, lat_chunks = 2048, blk_chunks = 2049, blk_kernels = 9, enc_pair = 1024, split_lanes = 1, chunks_per_group = 1,
        dense_mode = 1, ref_quirk = 0;
};

// what a call looks like to the planner
struct Shape {
    int codec = 0, esz = 1, D = 1;
    uint64_t nchunks = 0;                  // (encode: sprintz_mi355x_num_chunks(total_len, chunk_len))
    uint32_t chunk_len = 0;
    uint64_t total_len = 0;                // encode
    int noheader = 0, q = kQueryOff, general = 0;
    uint64_t col_stride = 0;
    int write_size = 1;                    // encode
    bool dense = false;                    // encode: a container was asked for (compact_tail.h)
    bool host_call = false;                // a single call that a workgroup-per-chunk kernel must end (entry.h: HostCall)
    unsigned src_lo = 0, slots_lo = 0, out_lo = 0, comp_lo = 0;   // the low four bits of the source, slot, output and container addresses
    uint64_t slot_stride = 0;
    uint64_t nranges = 0;                  // gather
    uint32_t rows = 0;                     // gather: rows of a range; rolling rows: the window W; project rows: the columns K of the output; derive rows: the forms K; FIR rows: the taps T
    uint64_t capacity = 0;                 // select: rows of the output
    // histogram, group-by: the uint32 entries of a workgroup's table (D x nbins, at most kHistMaxCounters; nbins x (D + 1), at most
    // kGroupByMaxCounters) and the most that one row can add to an entry (1; 2^W - 1).  0 entries: the mode has no table
    uint32_t table_entries = 0, table_row_max = 0;
    // the element bytes on the float side (4, or 2 for float16 / bfloat16): float rows' output element -- what every bound on output BYTES
    // counts in (project rows: the output element whatever it is, esz unconverted; derive rows and FIR rows: 4 for int32 and float32, 2 for the 16-bit floats) -- and, for an encode with q == kQueryFloat, the float
    // source's element; 0: the call has no float side
    int out_esz = 0;
};

struct Plan {
    int err = 0;                           // != 0: the call fails with this code and `what`; family stays -1
    const char* what = nullptr;
    int family = -1;                       // SPRINTZ_KF_*
    uint64_t grid = 0;
    uint64_t lds = 0;                      // dynamic LDS bytes (any_ndims.hip sizes its decoder's window itself: 0 here)
    int dp = 0, cpl = 0, ds = 0, log2DP = 0;
    bool exact = false, lowdim = false, fire = false;
    uint32_t lds_group_stride = 0, cap = 0, chunks_per_group = 1, lat_bound = 0;
    int vec_store = 0, norle = 0, raw = 0, quirk = 0;
    bool fused = false;                    // the encoder builds the container itself: grid + 1 zeroed words of d_tmp in front of it
    bool plain_memory = false;             // the output / the slots must be ordinary device memory (checked BEFORE err is reported, as the launch sites did)
    bool counters = false;                 // FIRE counters in stream-ordered scratch, nchunks x D x 4 bytes
    // histogram, group-by: where a workgroup's table of uint32 entries starts in its dynamic LDS (behind the groups' carves), and the
    // consecutive chunks a workgroup decodes -- 0 where their rows could wrap a 32-bit entry: such a launch adds in global memory
    uint32_t table_off = 0, wg_chunks = 0;
    RowDecGeom row{};
    BlkDecGeom blkd{};
    BlkEncGeom blke{};
};

inline Plan& plan_fail(Plan& p, int code, const char* what) { p.err = code; p.what = what; p.family = -1; return p; }
inline Plan& plan_take(Plan& p, int family, uint64_t grid, uint64_t lds)
{
    if (grid > 0x7fffffffull) return plan_fail(p, SPRINTZ_E_INVALID, "too many chunks for one launch");
    p.family = family; p.grid = grid; p.lds = lds;
    return p;
}

// (only 16-bit general-layout FIRE streams have the divergence: sprintz_xff_rle.cpp:893-901)
inline bool decode_ref_quirk(int codec, int esz, bool lowdim, const Knobs& k) { return esz == 2 && codec == SPRINTZ_CODEC_XFF && !lowdim && k.ref_quirk; }

// One chunk's working set of the workgroup-per-chunk kernels (decode_lat.h / encode_lat.h) must fit a workgroup's LDS: up to 16 KB of
// samples several workgroups share a CU (what the batch limits of SPRINTZ_OPT_LAT_CHUNKS were measured with); larger chunks -- up to
// ~40 KB of uint16, ~24 KB of uint8: 150 KB of LDS, a workgroup a CU -- only for batches that leave most CUs empty anyway (single calls)
inline bool lat_chunk_fits(bool encode, int esz, uint64_t nchunks, uint32_t chunk_len, int D)
{
    const uint64_t bytes = (uint64_t)chunk_len * esz;
    // (the 48 KB term never decides: both kernels keep 4 bytes an element of working set next to the stream -- 96 KB for 48 KB of uint16, 192 KB
    //  for uint8 -- so the 150 KB carve below refuses a chunk long before it: uint16 x 8 from 45 696 bytes on to decode, from 33 104 to encode
    //  (tests/dispatch_cases.py pins both sides).  It stays as the bound that keeps the 32-bit arithmetic of the carves far from a wrap)
    if (bytes > (48u << 10) || (bytes > kLatMaxChunkBytes && nchunks > 64)) return false;
    // the carve and the 16-bit position limit are checked for EVERY size: a shape whose working set does not fit goes to the
    // lane-per-column kernels instead of failing its launch
    const uint32_t bound = (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D);
    if (bound > 60000u) return false;                            // (stream positions travel in 16 bits between the kernels' phases)
    const uint32_t total = encode ? enc_lat_carve(bound, chunk_len, (uint32_t)D, (uint32_t)esz).total : lat_carve(bound, chunk_len, (uint32_t)D).total;
    return total <= 150u * 1024u;
}

// lanes of a workgroup-per-chunk kernel's column group, both directions (decode_lat.h / encode_lat.h, DP)
inline int lat_lanes(int esz, int D, bool lowdim)
{
    int ldp = 4;
    while (ldp < D) ldp <<= 1;
    if (esz == 1 && ldp < 8 && !lowdim) ldp = 8;
    return ldp;
}

// decode_fast.h's lanes per chunk, columns per lane and the LDS of one lane group (ring, apron, staging), for decode and gather
struct FastMap { int dp, cpl, ds, log2dp; uint32_t ring; };
inline FastMap decode_fast_map(int esz, int D, uint64_t cs, bool split)
{
    FastMap f{4, 1, 0, 0, 0};
    while (f.dp < D && f.dp < 64) f.dp <<= 1;
    while (f.dp * f.cpl < D) f.cpl <<= 1;                      // 2 / 4 columns per lane for D in 65..256
    // (for 65..96 columns <DP 32, CPL 3> keeps 84 % of the lanes busy instead of 62 % but holds 9 waves per CU
    //  instead of 12: measured slower, u8 D=80 1.29 -> 1.26 TB/s, u16 D=80 1.63 -> 1.34)
    // (two columns per lane at D = 8, i.e. <DP 4, CPL 2>, halves the lanes per chunk but not the LDS per chunk:
    //  8 waves per CU instead of 16, measured 0.494 vs 0.400 ms -- the doubled ILP does not replace the lost waves)
    // 8 bits, 65 .. 80 columns, plain row-major decode: 32 lanes x (a pair + a single column), two chunks a wavefront, the LDS
    // carve sized for 80 columns so that 12 wavefronts a CU stay resident (decode_fast.h, SPLIT)
    if (esz == 1 && D > 64 && D <= 80 && split) { f.dp = 32; f.cpl = 3; f.ds = 80; }
    // 16 bits, the same widths: 64 x 2 stays, with the carve of 80 columns (12.2 KB a chunk instead of 17.8: 12 waves a CU instead of 8)
    if (esz == 2 && D > 64 && D <= 80 && split) f.ds = 80;
    // (padding the stride by 16 / 32 / 48 bytes to move the groups' staging rows onto other banks: no change, 0.4225 ms each)
    f.ring = decode_fast_lds_bytes(8 * esz, f.dp, f.cpl, D, cs != 0 && f.cpl == 1, f.ds);
    while ((1 << f.log2dp) < f.dp) f.log2dp++;
    return f;
}

// more than 2 047 columns, FIRE (any_ndims.hip, "big"): the counters live in stream-ordered scratch
inline bool big_counters(Plan& p, const Shape& s)
{
    p.counters = s.codec == SPRINTZ_CODEC_XFF;
    if (p.counters && s.nchunks * (uint64_t)s.D * 4 > (1ull << 30)) {
        plan_fail(p, SPRINTZ_E_UNSUPPORTED, "more than 2047 columns, FIRE: the counters' scratch (nchunks x ndims x 4 bytes) is limited to 1 GiB a launch: split the batch");
        return false;
    }
    return true;
}

static_assert(kHistMaxCounters == SPRINTZ_HIST_MAX_COUNTERS, "the table's size is the header's cap");
static_assert(kGroupByMaxCounters == SPRINTZ_GBY_MAX_COUNTERS, "the table's size is the header's cap");
// histogram, group-by rows: a table entry takes at most one add a row of the workgroup's chunks, of at most row_max -- a count of 1, a
// sum of at most 2^W - 1 (a delta run's value x rows is the same bound) -- so wg_chunks x (chunk_len / D) x row_max must fit 32 bits;
// the table is merged once, at the kernel's end
inline uint32_t table_wg_chunks(uint64_t wg_chunks, uint32_t chunk_len, int D, uint32_t row_max)
{
    return wg_chunks * (uint64_t)(chunk_len / (uint32_t)D) * row_max <= 0xffffffffull ? (uint32_t)wg_chunks : 0u;
}

inline Plan plan_decode(const Shape& s, const Knobs& k)
{
    Plan p;
    const int D = s.D, esz = s.esz, codec = s.codec;
    const uint64_t nchunks = s.nchunks, cs = s.col_stride;
    const uint32_t chunk_len = s.chunk_len;
    const bool norle = codec >= SPRINTZ_CODEC_DELTA_NORLE;      // general layout for every ndims, generic kernels
    const bool lowdim = (s.general || norle) ? false : is_lowdim(esz, D);
    const Mapping m = choose_mapping(D, lowdim);
    const int DP = 1 << m.log2DP;
    p.lowdim = lowdim;
    p.fire = codec == SPRINTZ_CODEC_XFF || codec == SPRINTZ_CODEC_XFF_NORLE;
    p.log2DP = m.log2DP;
    p.cpl = m.cpl;
    p.norle = norle ? (codec == SPRINTZ_CODEC_XFF_NORLE ? 2 : 1) : 0;
    p.raw = codec == SPRINTZ_CODEC_BITPACK_NORLE ? 1 : 0;
    p.quirk = decode_ref_quirk(codec, esz, lowdim, k) ? 1 : 0;
    // float rows store elements of another size: the bytes a chunk slot of the output has are chunk_len x osz
    const bool flt = s.q == kQueryFloat;
    const int osz = flt ? s.out_esz : esz;

    // rolling rows (W in s.rows; s.out_esz the widest output element: 4 with the sum, else esz; s.out_lo the low bits of EVERY selected output).
    // decode_fast.h takes rows of whole 16-byte pieces -- gather's, select's and float rows' mappings -- with 16-byte aligned outputs, within the
    // descriptors' reach counted in OUTPUT bytes (out_esz), where the chunks' history rings (geom.h: roll_ring_bytes) fit behind the groups' carves:
    // (f.ring + roll_ring) x groups <= kHistFastLdsBudget -- on the one-column-a-lane mappings (up to 64 columns): with two and four columns a lane
    // hipcc kept the block's results in scratch, for min and max as for the sum, so those mappings are not instantiated.  min, max and sum alike: the
    // sum leaves as 32 / W element-type planes through the plain staging, free of scratch on every mapping kept.  Everything else runs the generic
    // kernel, whose launch LDS is the rings alone and which stores element by element; rings that do not fit a workgroup's 160 KB there are refused
    // (roll_shape_max_window).  decode_uni.h is not taught the mode.
    if (s.q == kQueryRolling) {
        if (D > 512 || norle || cs) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "rolling_rows: the RLE codecs, row-major, at most 512 columns");
        if (s.rows < 8 || s.rows % 8) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "rolling_rows: window_rows must be a multiple of 8, at least 8");
        const uint64_t ring = roll_ring_bytes(s.rows, D, esz);
        const int osz = s.out_esz ? s.out_esz : esz;
        const FastMap f = decode_fast_map(esz, D, 0, false);
        const uint64_t fgroups = (uint64_t)(kThreads / f.dp);
        const bool fast = !lowdim && !s.noheader && f.cpl == 1 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast &&
                          ((uint64_t)D * esz) % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                          (uint64_t)chunk_len * osz * 64 * 64 < 0xf0000000ull && ((uint64_t)f.ring + ring) * fgroups <= kHistFastLdsBudget;
        if (fast) {
            p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
            p.exact = D == f.dp * f.cpl;
            p.log2DP = f.log2dp;
            p.lds_group_stride = f.ring;
            p.vec_store = 1;
            p.chunks_per_group = (uint32_t)k.chunks_per_group;
            p.table_off = f.ring * (uint32_t)fgroups;
            const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
            return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, ((uint64_t)f.ring + ring) * fgroups);
        }
        const uint32_t groups = (uint32_t)(kThreads / DP);
        if (s.rows > roll_shape_max_window(D, esz, !lowdim))
            return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "rolling_rows: window_rows must be a multiple of 8 whose history rings fit a workgroup's LDS (roll_shape_max_window)");
        p.lds_group_stride = (uint32_t)ring;
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, (uint64_t)p.lds_group_stride * groups);
    }

    // cumulative rows (s.out_esz the widest output element: sum_bytes with the sum, else esz; s.out_lo the low bits of EVERY selected output).
    // decode_fast.h takes what it takes for rolling rows, without the rings: rows of whole 16-byte pieces on the one-column-a-lane mappings (8 .. 64
    // columns), 16-byte aligned outputs, within the descriptors' reach counted in OUTPUT bytes (out_esz: the int64 sum's offsets are eight times the
    // element's at 8 bits).  Two and four columns a lane are not instantiated, as for rolling rows; everything else -- the low-dim shapes too:
    // decode_uni.h is not taught the mode -- runs the generic kernel, which stores element by element at 64-bit addresses and stages nothing.
    if (s.q == kQueryCumulative) {
        if (D > 512 || norle || cs) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "cumulative_rows: the RLE codecs, row-major, at most 512 columns");
        const int cosz = s.out_esz ? s.out_esz : esz;
        const FastMap f = decode_fast_map(esz, D, 0, false);
        const uint64_t fgroups = (uint64_t)(kThreads / f.dp);
        const bool fast = !lowdim && !s.noheader && f.cpl == 1 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast &&
                          ((uint64_t)D * esz) % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                          (uint64_t)chunk_len * cosz * 64 * 64 < 0xf0000000ull;
        if (fast) {
            p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
            p.exact = D == f.dp * f.cpl;
            p.log2DP = f.log2dp;
            p.lds_group_stride = f.ring;
            p.vec_store = 1;
            p.chunks_per_group = (uint32_t)k.chunks_per_group;
            const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
            return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, (uint64_t)f.ring * fgroups);
        }
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, 0);
    }

    // project rows (K in s.rows; s.out_esz the bytes of an output element: esz for the element type, 4 / 2 for the floats).  A chunk's R = chunk_len / D
    // rows leave as R x K elements from output element c x R x K on.  decode_fast.h takes, on its one-column-a-lane mappings (up to 64 columns), every
    // shape the plain decode takes there whose PROJECTED block, 8 K esz bytes, is a whole number of 16-byte store pieces -- every K at 16 bits, the even
    // ones at 8 -- with the reach of the store descriptor counted in projected output bytes.  A chunk's projected slot need not be a multiple of 16
    // bytes: its pieces are then stored at addresses aligned to the output element alone.  With two and four columns a lane the mode is not instantiated
    // (plan.h names no such mapping), and everything else runs the generic kernel, which stores element by element at 64-bit addresses and stages nothing.
    if (s.q == kQueryProject) {
        const uint32_t K = s.rows;
        if (K == 0 || K > (uint32_t)D) return plan_fail(p, SPRINTZ_E_INVALID, "project_rows: ncolumns must be in 1 .. ndims");
        if (D > 512 || norle || cs) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "project_rows: the RLE codecs, row-major, at most 512 columns");
        const int posz = s.out_esz ? s.out_esz : esz;
        const uint64_t slot_bytes = (uint64_t)(chunk_len / (uint32_t)D) * K * (uint64_t)posz;      // a chunk's projected output
        const FastMap f = decode_fast_map(esz, D, 0, false);
        const bool fast = !lowdim && !s.noheader && f.cpl == 1 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast &&
                          // the plain decode's terms for the shape (whole 16-byte pieces a block and a chunk, a 16-byte aligned output) ...
                          ((uint64_t)8 * D * esz) % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                          // ... and the projection's: whole pieces a projected block, the wave's chunks within reach of 32-bit offsets
                          ((uint64_t)8 * K * esz) % 16 == 0 && slot_bytes * 64 * 64 < 0xf0000000ull;
        if (fast) {
            p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
            p.exact = D == f.dp * f.cpl;
            p.log2DP = f.log2dp;
            p.lds_group_stride = f.ring;
            p.vec_store = 1;
            p.chunks_per_group = (uint32_t)k.chunks_per_group;
            const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
            return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, (uint64_t)f.ring * (kThreads / f.dp));
        }
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, 0);
    }

    // derive rows (K in s.rows; s.out_esz the bytes of an output element: 4 for int32 and float32, 2 for float16 / bfloat16).  A chunk's R = chunk_len / D
    // rows leave as R x K values from output element c x R x K on.  decode_fast.h takes, on its one-column-a-lane mappings (up to 64 columns), every shape
    // the plain decode takes there: the DERIVED block, 8 K osz bytes, is a whole number of 16-byte store pieces for every K, the reach of the store
    // descriptor is counted in derived output bytes, and the output must be 16-byte aligned.  The group's staging is sized for the derived block where
    // that is more than the decoded one, and the workgroup's table of weights ([K][D] pairs of words) sits behind the groups' carves (table_off), both
    // within the budget the histogram's launch has.  With two and four columns a lane the mode is not instantiated (a lane would keep the block's rows of
    // every column in registers next to the plain decode's state; plan.h names no such mapping), and everything else -- the low-dim shapes too:
    // decode_uni.h is not taught the mode -- runs the generic kernel, which stores value by value at 64-bit addresses and stages nothing.
    if (s.q == kQueryDerive) {
        const uint32_t K = s.rows;
        if (K == 0 || K > kDeriveMaxForms) return plan_fail(p, SPRINTZ_E_INVALID, "derive_rows: nforms must be in 1 .. 16");
        if (D > 512 || norle || cs) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "derive_rows: the RLE codecs, row-major, at most 512 columns");
        const int dosz = s.out_esz ? s.out_esz : 4;
        const uint64_t slot_bytes = (uint64_t)(chunk_len / (uint32_t)D) * K * (uint64_t)dosz;      // a chunk's derived output
        const FastMap f = decode_fast_map(esz, D, 0, false);
        const uint64_t fgroups = (uint64_t)(kThreads / f.dp);
        const uint64_t staged = ((uint64_t)8 * D * esz + 15) & ~15ull, derived = (uint64_t)8 * K * dosz;
        const uint64_t dstride = (uint64_t)f.ring + (derived > staged ? derived - staged : 0);
        const uint64_t wtable = (uint64_t)K * D * 8;
        const bool fast = !lowdim && !s.noheader && f.cpl == 1 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast &&
                          // the plain decode's terms for the shape (whole 16-byte pieces a block and a chunk, a 16-byte aligned output) ...
                          ((uint64_t)8 * D * esz) % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                          // ... and the derivation's: the wave's chunks within reach of 32-bit offsets, staging and table within the LDS budget
                          slot_bytes * 64 * 64 < 0xf0000000ull && dstride * fgroups + wtable <= kHistFastLdsBudget;
        if (fast) {
            p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
            p.exact = D == f.dp * f.cpl;
            p.log2DP = f.log2dp;
            p.lds_group_stride = (uint32_t)dstride;
            p.vec_store = 1;
            p.chunks_per_group = (uint32_t)k.chunks_per_group;
            p.table_off = (uint32_t)(dstride * fgroups);
            const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
            return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, dstride * fgroups + wtable);
        }
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, 0);
    }

    // FIR rows (T in s.rows; s.out_esz the bytes of an output element: 4 for int32 and float32, 2 for float16 / bfloat16).  The history is rolling rows'
    // ring with W replaced by Wh = fir_history_rows(T).  decode_fast.h takes the shapes it takes for rolling rows -- rows of whole 16-byte pieces on the
    // one-column-a-lane mappings (8 .. 64 columns), a 16-byte aligned output, within the descriptor's reach counted in OUTPUT bytes -- where the chunks'
    // rings behind the groups' carves and the workgroup's table of taps ([T][D] int32) behind the rings fit the budget the histogram's launch has:
    // (f.ring + ring) x groups + 4 T D <= kHistFastLdsBudget.  Two and four columns a lane are not instantiated, as for rolling rows.  Everything else runs
    // the generic kernel, whose launch LDS is the rings alone, which reads its taps from global memory and stores element by element; a history that does
    // not fit a workgroup's 160 KB there is refused (fir_shape_max_taps).  decode_uni.h is not taught the mode.
    if (s.q == kQueryFir) {
        const uint32_t T = s.rows;
        if (D > 512 || norle || cs) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "fir_rows: the RLE codecs, row-major, at most 512 columns");
        if (T < 1 || T > kFirMaxTaps) return plan_fail(p, SPRINTZ_E_INVALID, "fir_rows: ntaps must be in 1 .. 256");
        if (T - 1u > chunk_len / (uint32_t)D) return plan_fail(p, SPRINTZ_E_INVALID, "fir_rows: ntaps - 1 must not exceed the rows of a chunk, chunk_len / ndims");
        const uint64_t ring = roll_ring_bytes(fir_history_rows(T), D, esz);
        const int fosz = s.out_esz ? s.out_esz : 4;
        const FastMap f = decode_fast_map(esz, D, 0, false);
        const uint64_t fgroups = (uint64_t)(kThreads / f.dp);
        const uint64_t ttable = (uint64_t)T * D * 4;
        const bool fast = !lowdim && !s.noheader && f.cpl == 1 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast &&
                          ((uint64_t)D * esz) % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                          (uint64_t)chunk_len * fosz * 64 * 64 < 0xf0000000ull && ((uint64_t)f.ring + ring) * fgroups + ttable <= kHistFastLdsBudget;
        if (fast) {
            p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
            p.exact = D == f.dp * f.cpl;
            p.log2DP = f.log2dp;
            p.lds_group_stride = f.ring;
            p.vec_store = 1;
            p.chunks_per_group = (uint32_t)k.chunks_per_group;
            p.table_off = f.ring * (uint32_t)fgroups;
            const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
            return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, ((uint64_t)f.ring + ring) * fgroups + ttable);
        }
        const uint32_t groups = (uint32_t)(kThreads / DP);
        if (T > fir_shape_max_taps(D, esz, !lowdim))
            return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "fir_rows: ntaps must leave the history rings within a workgroup's LDS (fir_shape_max_taps)");
        p.lds_group_stride = (uint32_t)ring;
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, (uint64_t)p.lds_group_stride * groups);
    }

    // 513 .. 2047 columns: one workgroup per chunk (any_ndims.hip) -- the RLE codecs, row-major, plain decode
    if (D > 512) {
        if (norle || cs || s.q != kQueryOff) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "more than 512 columns: the RLE codecs, row-major, without query only");
        if (nchunks > 0x7fffffffull) return plan_fail(p, SPRINTZ_E_INVALID, "too many chunks for one launch");
        if (D > 2047) {                                        // column tiles; the FIRE counters in stream-ordered scratch (any_ndims.hip, "big")
            p.plain_memory = true;
            if (!big_counters(p, s)) return p;
            return plan_take(p, SPRINTZ_KF_DEC_BIG, nchunks, 0);
        }
        return plan_take(p, SPRINTZ_KF_DEC_ANY, nchunks, 0);
    }

    // batches whose chunks are too short for a stream group: header check + copy (verbatim_decode_kernel)
    // (only where a chunk cannot hold a group at all, chunk_len < 16 D: a stream of 16 D <= chunk_len < 128 elements that announces
    //  groups is one the reference ENCODER never writes but its decoder reads -- that one goes to the decoders below)
    if (!norle && !lowdim && !s.noheader && !cs && s.q == kQueryOff && chunk_len < 16u * (uint32_t)D && !k.no_fast)
        return plan_take(p, SPRINTZ_KF_DEC_VERBATIM, (nchunks * 64 + kThreads - 1) / kThreads, 0);

    // LDS-transposed 16-byte stores need every 8 x D block of the output 16-byte aligned
    const size_t blk_bytes = (size_t)8 * D * esz;
    const size_t stride = ((blk_bytes + 15) & ~(size_t)15) + 16;     // +16: spread groups over LDS banks
    const size_t groups_per_block = kThreads / DP;
    size_t shmem = 0;
    if (!cs && blk_bytes % 16 == 0 && (query_reduce_only(s.q) || (s.out_lo % 16) == 0) && ((uint64_t)chunk_len * esz) % 16 == 0 &&
        stride * groups_per_block <= 64 * 1024) {
        p.vec_store = 1;
        p.lds_group_stride = (uint32_t)stride;
        shmem = stride * groups_per_block;
    }

    // Fast path (decode_fast.h): general layout, one column per lane, headered stream,
    // vector stores legal, and the power-of-two group at least half full.
    // (32-bit offsets inside one wavefront's span of the output)
    // and chunks not much shorter than the read-ahead ring (it is filled before the first header is parsed)
    const FastMap f = decode_fast_map(esz, D, cs, !cs && s.q == kQueryOff && k.split_lanes);
    const bool fast_common = !lowdim && !p.raw && !s.noheader && D <= 256 && 2 * D > f.dp * f.cpl && (uint64_t)chunk_len * esz * 2 >= f.ring && !k.no_fast;
    // column-major: a lane's 8 samples per block are one aligned 16-byte (8-byte) piece of its column
    const bool fast = cs ? fast_common && s.q == kQueryOff && cs % 8 == 0 && (chunk_len / (uint32_t)D) % 8 == 0 &&
                               (s.out_lo % 16) == 0 && (uint64_t)D * cs * esz < 0xf0000000ull
                         : fast_common && p.vec_store && (uint64_t)chunk_len * osz * 64 * 64 < 0xf0000000ull &&
                               // float rows: rows of whole 16-byte INPUT pieces, so that a lane's store piece holds the same columns in every block
                               // (the 16-byte aligned output is vec_store's term; the reach above counts OUTPUT bytes)
                               (!flt || ((uint64_t)D * esz) % 16 == 0) &&
                               // select rows: the shapes a filter takes here, with rows of whole 16-byte store pieces (a piece lies in ONE row, as
                               // for the gather) and an output -- `capacity` rows from a 16-byte aligned start -- within reach of the store
                               // descriptor's 32-bit offsets (the quotient: capacity is any 64-bit number)
                               (s.q != kQuerySelect || (((uint64_t)D * esz) % 16 == 0 && (s.out_lo % 16) == 0 &&
                                                        s.capacity <= (0xf0000000ull - 1) / ((uint64_t)D * esz)));
    // small batches: one WORKGROUP per chunk (decode_lat.h) -- a chunk's 40 dependent group steps on one lane group take 50 us
    // however few chunks there are; split into a header walk, parallel bit extraction, the bare recurrence and a prefix sum it is ~13
    if (!norle && !s.noheader && !cs && !p.quirk && s.q == kQueryOff && D <= 64 &&
        lat_chunk_fits(false, esz, nchunks, chunk_len, D) && chunk_len >= 16u * (uint32_t)D && (s.out_lo % 16) == 0 &&
        (nchunks == 1 || ((uint64_t)chunk_len * esz) % 16 == 0) &&      // (a chunk's output starts 16-byte aligned; its end may lie anywhere)
        // (about one round of workgroups on the chip is where it wins: 5 a CU at 8 columns -- measured 33 vs 47 us at 1 250 chunks, 41 vs 47
        //  at 2 048, 59 vs 47 at 3 072; with more columns a chunk has fewer groups to walk and the lane-per-column kernel catches up
        //  sooner: 32 columns 11.6 vs 14.7 at 640 chunks, 19.7 vs 14.8 at 1 250 -- a third of the limit from 17 columns on)
        nchunks <= (uint64_t)k.lat_chunks / (D > 16 ? 3u : 1u) && !k.no_fast) {     // (raw is a run-less codec)
        p.dp = lat_lanes(esz, D, lowdim);
        p.lat_bound = (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D);
        return plan_take(p, SPRINTZ_KF_DEC_LAT, nchunks, lat_carve(p.lat_bound, chunk_len, (uint32_t)D).total);
    }
    // large batches of the DELTA codec, general layout, rows of whole dwords: a lane per dword-wide column group, blocks in order (decode_row.h)
    if (k.blk_chunks > 0 && (k.blk_kernels & 8) && nchunks >= (uint64_t)k.blk_chunks && codec == SPRINTZ_CODEC_DELTA && !lowdim && !s.noheader && !cs &&
        s.q == kQueryOff && !s.host_call && (s.out_lo % 4) == 0 && (s.comp_lo % 4) == 0 && !k.no_fast) {
        const RowDecGeom g = row_dec_geom((uint32_t)esz, chunk_len, (uint32_t)D);
        // where it wins (tools/blk_shapes.py, profiles/r6_blk_shapes.txt; 10 KB chunks, ms against the lane-per-column kernels): 8-bit rows of 32 / 48 / 64 / 80 /
        // 128 / 256 columns 0.153 / 0.202 / 0.121 / 0.132 / 0.136 / 0.187 against 0.172 / 0.237 / 0.184 / 0.172 / 0.155 / 0.539; where it does not: 16 8-bit columns
        // (4 lanes a chunk) 0.233 against 0.182, and 16-bit elements -- two fields a dword carry the same per-row work as four -- 8 / 16 / 24 / 128 columns 0.129 /
        // 0.103 / 0.171 / 0.186 against 0.114 / 0.096 / 0.136 / 0.132 (32 and 64 columns level).  Mask bit 4 takes every shape the kernel fits (tests).
        const bool wins = (esz == 1 && g.U >= 8u) || (k.blk_kernels & 16);
        // (32-bit offsets into the OUTPUT inside the kernel: a batch that decodes to 4 GB or more goes to the kernels below.  The container may lie
        //  anywhere -- d_offsets are the caller's, and a stream's base is a 64-bit address there)
        const bool below_4g = (uint64_t)nchunks * chunk_len * esz < 0xf0000000ull;
        if (g.ok && below_4g && wins) {
            p.row = g;
            return plan_take(p, SPRINTZ_KF_DEC_ROW, (nchunks + 4ull * g.G - 1) / (4ull * g.G), 0);
        }
    }
    // ... or the block-parallel decoder (decode_blk.h)
    if (k.blk_chunks > 0 && (k.blk_kernels & 2) && nchunks >= (uint64_t)k.blk_chunks && codec == SPRINTZ_CODEC_DELTA && !lowdim && !s.noheader && !cs &&
        s.q == kQueryOff && !s.host_call && (s.out_lo % 16) == 0 && !k.no_fast) {
        const BlkDecGeom g = blk_dec_geom((uint32_t)esz, chunk_len, (uint32_t)D, (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D));
        if (g.ok) {
            p.blkd = g;
            return plan_take(p, SPRINTZ_KF_DEC_BLK, (nchunks + g.CPW - 1) / g.CPW, g.total);
        }
    }
    // histogram, group-by rows: the workgroup's table sits behind the groups' carves, and both must fit the launch's LDS budget
    const uint64_t table_bytes = 4ull * s.table_entries;
    if (fast && (table_bytes == 0 || (uint64_t)f.ring * (kThreads / f.dp) + table_bytes <= kHistFastLdsBudget)) {
        p.dp = f.dp; p.cpl = f.cpl; p.ds = f.ds;
        p.exact = D == f.dp * f.cpl;
        p.log2DP = f.log2dp;
        p.lds_group_stride = f.ring;
        // consecutive chunks per lane group.  Measured on MI355X (cfg2, 131072 chunks): k = 1 / 2 / 4 /
        // 8 -> 0.498 / 0.496 / 0.510 / 0.560 ms: one generation of lock-stepped groups is no faster
        // than four staggered ones, so the default stays at one chunk per group (env knob for tuning).
        p.chunks_per_group = (uint32_t)k.chunks_per_group;
        const uint64_t ngroups_launch = (nchunks + p.chunks_per_group - 1) / p.chunks_per_group;
        if (table_bytes) {
            p.table_off = f.ring * (uint32_t)(kThreads / f.dp);
            p.wg_chunks = table_wg_chunks((uint64_t)(kThreads / f.dp) * p.chunks_per_group, chunk_len, D, s.table_row_max);
        }
        return plan_take(p, SPRINTZ_KF_DEC_FAST, (ngroups_launch * (uint64_t)f.dp + kThreads - 1) / kThreads, (uint64_t)f.ring * (kThreads / f.dp) + table_bytes);
    }
    // univariate streams: one lane per chunk, LDS ring in, quad-transposed 64-byte bursts out (decode_uni.h)
    // (and the other low-dim shapes: 2 columns, 3 and 4 at 8 bits)
    // (decode_uni.h is not taught to select or to aggregate rows, nor the histogram, nor the moments, nor the group-by, nor the extrema, nor the linear filter, nor the segments, nor float rows (rolling rows left above): those shapes go to the generic kernel)
    if (lowdim && (D <= 2 || esz == 1) && !s.noheader && !cs && s.q != kQuerySelect && s.q != kQueryAggregate && s.q != kQueryHistogram && s.q != kQueryMoments && s.q != kQueryGroupBy && s.q != kQueryExtrema && s.q != kQueryLinear && s.q != kQuerySegment && s.q != kQueryFloat && !k.no_fast) return plan_take(p, SPRINTZ_KF_DEC_UNI, (nchunks + 255) / 256, 0);
    if (table_bytes) {                                         // nothing is staged: the table is the launch's LDS
        p.wg_chunks = table_wg_chunks((uint64_t)(kThreads / DP), chunk_len, D, s.table_row_max);
        return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, table_bytes);
    }
    if (flt) {                                                 // every sample leaves converted, at a plain 64-bit address: nothing is staged
        p.vec_store = 0;
        p.lds_group_stride = 0;
        shmem = 0;
    }
    return plan_take(p, SPRINTZ_KF_DEC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, shmem);
}

// gather rows: decode_fast.h for the shapes the decode takes there, with rows of whole 16-byte store pieces, and both the container and
// the output within reach of one descriptor's 32-bit offsets.  The container's size is on the device; every container this library writes
// stays below nchunks * (compress_bound + alignment).  Everything else goes to the generic kernel: plain 64-bit addresses.
inline uint64_t gather_pieces(uint32_t rows, uint32_t R) { return ((uint64_t)rows + R - 2) / R + 1; }   // the most chunks a range of `rows` rows can touch, R rows a chunk
inline Plan plan_gather(const Shape& s, const Knobs& k)
{
    Plan p;
    const int D = s.D, esz = s.esz;
    const uint64_t slots = s.nranges * gather_pieces(s.rows, s.chunk_len / (uint32_t)D);
    const bool lowdim = is_lowdim(esz, D);
    const Mapping m = choose_mapping(D, lowdim);
    p.lowdim = lowdim;
    p.fire = s.codec == SPRINTZ_CODEC_XFF;
    p.log2DP = m.log2DP;
    p.cpl = m.cpl;
    p.quirk = decode_ref_quirk(s.codec, esz, lowdim, k) ? 1 : 0;
    const FastMap f = decode_fast_map(esz, D, 0, false);
    const uint64_t out_bytes = s.nranges * (uint64_t)s.rows * (uint64_t)D * esz;          // (nranges * P <= 2^40 and rows <= P * R: no wrap)
    const uint64_t comp_bound = s.nchunks * (uint64_t)(compress_bound(esz, s.chunk_len, (uint16_t)D) + 64);
    const bool fast = !lowdim && D <= 256 && 2 * D > f.dp * f.cpl && (uint64_t)s.chunk_len * esz * 2 >= f.ring && ((uint64_t)D * esz) % 16 == 0 &&
                      (s.out_lo % 16) == 0 && out_bytes < 0xf0000000ull && s.nchunks < (1ull << 32) && comp_bound < 0xf0000000ull && !k.no_fast;
    if (fast) {
        p.dp = f.dp; p.cpl = f.cpl;
        p.exact = D == f.dp * f.cpl;
        p.log2DP = f.log2dp;
        p.lds_group_stride = f.ring;
        plan_take(p, SPRINTZ_KF_GATHER_FAST, (slots * (uint64_t)f.dp + kThreads - 1) / kThreads, (uint64_t)f.ring * (kThreads / f.dp));
    } else {
        plan_take(p, SPRINTZ_KF_GATHER_GENERIC, ((slots << m.log2DP) + kThreads - 1) / kThreads, 0);
    }
    if (p.err) p.what = "gather_rows: too many pieces for one launch";
    return p;
}

inline Plan plan_encode(const Shape& s, const Knobs& k)
{
    Plan p;
    const int D = s.D, esz = s.esz, codec = s.codec;
    const uint64_t nchunks = s.nchunks, col_stride = s.col_stride;
    const uint32_t chunk_len = s.chunk_len;
    const bool norle = codec >= SPRINTZ_CODEC_DELTA_NORLE;
    const bool lowdim = (norle || s.general) ? false : is_lowdim(esz, D);
    const Mapping m = choose_mapping(D, lowdim);
    const int DP = 1 << m.log2DP;
    p.lowdim = lowdim;
    p.fire = codec == SPRINTZ_CODEC_XFF || codec == SPRINTZ_CODEC_XFF_NORLE;
    p.log2DP = m.log2DP;
    p.cpl = m.cpl;
    p.norle = norle ? (codec == SPRINTZ_CODEC_XFF_NORLE ? 2 : 1) : 0;
    p.raw = codec == SPRINTZ_CODEC_BITPACK_NORLE ? 1 : 0;
    // a float source (q == kQueryFloat, out_esz the bytes of a source float; quant.h): only the kernels that are taught to quantise while they
    // load -- encode_wide.h's (enc_pair, enc_wide, enc_split) and the generic one -- for the RLE codecs, row-major, up to 512 columns
    const bool flt = s.q == kQueryFloat;
    // (encode_wide.h keeps the parameters of a block's 8 D elements in LDS, once a workgroup, behind the groups' carves: 64 D bytes)
    const uint64_t qtab = flt ? 64ull * (uint64_t)D : 0;
    if (flt && (D > 512 || norle || col_stride)) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "a float source: the RLE codecs, row-major, at most 512 columns");
    // 513 .. 2047 columns: one workgroup per chunk, the window holds one stream group (any_ndims.hip)
    if (D > 512) {
        if (norle || col_stride) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "more than 512 columns: the RLE codecs, row-major only");
        if (nchunks > 0x7fffffffull) return plan_fail(p, SPRINTZ_E_INVALID, "too many chunks for one launch");
        if (D > 2047) {                                        // column tiles, fields OR-ed straight into the zeroed slot (any_ndims.hip, "big")
            if (s.slot_stride % 16 || (s.slots_lo & 15)) return plan_fail(p, SPRINTZ_E_INVALID, "more than 2047 columns: slots must be 16-byte aligned and a multiple of 16 bytes");
            p.plain_memory = true;
            if (!big_counters(p, s)) return p;
            return plan_take(p, SPRINTZ_KF_ENC_BIG, nchunks, 0);
        }
        p.cap = ((uint32_t)group_bytes_max(esz, D) + 64u + 15u) & ~15u;
        return plan_take(p, SPRINTZ_KF_ENC_ANY, nchunks, p.cap);
    }
    // the generic kernel's window is a power-of-two RING flushed in 16-byte pieces; the kernels that flush whole 128-byte lines
    // (encode_fast.h, encode_wide.h) need that much more room in front of the write position: cap_drain (theirs alone -- added
    // to every encoder it doubled the generic ring wherever the group sat just under a power of two)
    p.cap = next_pow2((uint32_t)group_bytes_max(esz, D) + 48u);
    const uint32_t cap_drain = next_pow2((uint32_t)group_bytes_max(esz, D) + 48u + (uint32_t)(SPRINTZ_ENC_DRAIN_ALIGN - 16));
    const size_t shmem = ((size_t)p.cap + 16) * (kThreads / DP);
    if (shmem > 160 * 1024) return plan_fail(p, SPRINTZ_E_UNSUPPORTED, "ndims too large for the LDS output ring");

    // Fast path (encode_fast.h): general layout, one column per lane, every 8 x D input
    // block 16-byte aligned, the power-of-two group at least half full.
    int fdp = 4;
    while (fdp < D) fdp <<= 1;
    const size_t blk_bytes = (size_t)8 * D * esz;
    const bool fast_common = !lowdim && !p.raw && D <= 64 && 2 * D > fdp && (s.src_lo % 16) == 0 && !k.no_fast;
    // (column-major: the burst loads of encode_fast.h and encode_wide.h keep the stride as a 32-bit element count -- a stride of 2^32 elements
    //  or more goes to the generic kernel, whose stride is 64 bits wide)
    const bool cm_reach = col_stride <= 0xffffffffull;
    const bool fast = col_stride ? fast_common && col_stride % 8 == 0 && (chunk_len / (uint32_t)D) % 8 == 0 && cm_reach
                                 : fast_common && blk_bytes % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0;
    // small batches: one WORKGROUP per chunk (encode_lat.h), the counterpart of decode_lat.h -- 90 us for ONE 10 KB chunk on a lane
    // group, ~20 with the coefficient chain and the RLE state machine as the only serial parts (the container, if one was asked
    // for, is then built by the scan + copy passes: fused stays false)
    if (!flt && !norle && !col_stride && D <= 64 && lat_chunk_fits(true, esz, nchunks, chunk_len, D) &&
        (s.src_lo % 16) == 0 && (nchunks == 1 || ((uint64_t)chunk_len * esz) % 16 == 0) && s.slot_stride % 16 == 0 && (s.slots_lo % 16) == 0 &&
        // (a chunk is read in 16-byte pieces from a 16-byte aligned start: the last piece may reach past its end, never past the piece that holds its last byte)
        // (the encoder's crossover sits higher than the decoder's -- the lane-per-column encoders take ~100 us (uint16 x 8) / ~175 us (uint8 x 8)
        //  for ANY batch up to ~16 000 chunks: 75 vs 100 us at 3 072 chunks, 105 vs 101 at 4 096; 32 columns: 24 vs 26 at 1 024 -- tools/lat_sweep_enc.py)
        nchunks <= (uint64_t)k.lat_chunks * (D > 16 ? 1u : 3u) / (D > 16 ? 3u : 2u) && !k.no_fast) {
        p.dp = lat_lanes(esz, D, lowdim);
        p.lat_bound = (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D);
        return plan_take(p, SPRINTZ_KF_ENC_LAT, nchunks, enc_lat_carve(p.lat_bound, chunk_len, (uint32_t)D, (uint32_t)esz).total);
    }
    // large batches of the DELTA codec, general layout, rows of whole 16-byte pieces: the block-parallel encoder (encode_blk.h) -- a thread
    // per (block, 16-byte row piece), the RLE state machine as scans; the container, if one was asked for, by the scan + copy passes.
    // (The container inside this launch -- images flushed straight to their place, found by compact_tail.h's chained scan -- was built and
    //  measured on BASELINE config 3 at 10 KB, 17 476 workgroups of three chunks: 0.296 ms against 0.267 for the launches in a row.  Taken
    //  apart: no scan, no tickets 0.177; tickets alone +0.070 (17 476 atomics on one word); the look-back alone +0.089 with 256 predecessors
    //  a hop, +0.114 with 1 024 -- a workgroup that lives 10 us waits for the slowest of a thousand resident predecessors with 33 KB of LDS
    //  held.  The tail pays from 64 chunks a workgroup on, as on the lane-per-column kernels.
    //  Second form: a workgroup takes 16 / 32 / 64 chunks in passes of three and ends with compact_tail.h's dense_tail (slot -> container copy, one
    //  chained-scan step per workgroup): 0.352 / 0.369 / 0.432 ms against 0.280 on the same box -- the looped kernel needs 149 registers (3 waves a
    //  SIMD instead of 4) and 820 - 3 277 workgroups are one to three cohorts: the tails do not hide behind anybody's encoding.
    //  Third form, priced before it was built: encoders that never wait -- they flush to their slots with write-through (sc0 sc1) stores, wait for
    //  them and add their size to their block's word; the block's last finisher finds the block's place (a look-back over a few hundred blocks) and
    //  copies it.  The encoder's side alone (the stores, the s_waitcnt, one atomic a chunk; no placement at all) measured 0.302 against 0.270 ms for
    //  the whole compress call: a third of the 0.098 ms the scan + copy launches cost is gone before the placers' copies and the last block's tail.)
    if (!flt && k.blk_chunks > 0 && (k.blk_kernels & 1) && nchunks >= (uint64_t)k.blk_chunks && codec == SPRINTZ_CODEC_DELTA && !lowdim && !col_stride && !s.host_call && s.write_size &&
        (s.src_lo % 16) == 0 && s.slot_stride % 16 == 0 && (s.slots_lo % 16) == 0 && !k.no_fast) {
        const BlkEncGeom g = blk_enc_geom((uint32_t)esz, chunk_len, (uint32_t)D, (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D));
        if (g.ok) {
            p.blke = g;
            return plan_take(p, SPRINTZ_KF_ENC_BLK, (nchunks + g.CPW - 1) / g.CPW, g.total);
        }
    }
    // the same for univariate streams of the low-dim layout (BASELINE config 1): a thread per 16 bytes of the series
    if (!flt && k.blk_chunks > 0 && (k.blk_kernels & 4) && nchunks >= (uint64_t)k.blk_chunks && codec == SPRINTZ_CODEC_DELTA && lowdim && D == 1 && !col_stride && !s.host_call && s.write_size &&
        (s.src_lo % 16) == 0 && s.slot_stride % 16 == 0 && (s.slots_lo % 16) == 0 && !k.no_fast) {
        const BlkEncGeom g = blk_enc_uni_geom((uint32_t)esz, chunk_len, (uint32_t)compress_bound(esz, chunk_len, (uint16_t)D));
        if (g.ok) {
            p.blke = g;
            return plan_take(p, SPRINTZ_KF_ENC_BLK_UNI, (nchunks + g.CPW - 1) / g.CPW, g.total);
        }
    }
    // the container built inside the launch (compact_tail.h): every kernel of encode_fast.h / encode_wide.h carries the tail
    // (column-major sources keep the two-launch path: with the tail in encode_fast<CM> BASELINE config 5 took 0.089 instead of 0.076 ms, its
    //  8 M-row form 0.407 instead of 0.359 -- eight chunks a workgroup make the chained scan eight times as long per byte as sixty-four do)
    //  Measured likewise on the row-major kernels: 8 uint16 columns (64 chunks a workgroup) 0.661 with the tail, 0.670 without; 16 columns (32 chunks)
    //  0.148 / 0.142; 64 columns (8) 0.158 / 0.144; BASELINE config 3 at 10 KB (8) 0.431 / 0.408 -- the tail pays from 64 chunks a workgroup on.
    auto fuses = [&](size_t groups) { return s.dense && groups == 64 && !col_stride; };
    // two columns per lane for narrow row-major streams too (encode_wide.h with 4 .. 32 lanes a chunk): fewer instructions per sample
    // than encode_fast.h's one column per lane on every shape measured (tools/enc_pair_sweep.sh: -6 % .. -35 %)
    // (not for a handful of chunks: there a chunk's latency is what counts, and half the lanes per chunk make it longer -- a single 10 KB
    //  sprintz_compress_xff_16b call 127 us against 111 with one column per lane; from a thousand chunks on the two are level or better)
    // (column-major sources too: encode_fast.h's bursts, two columns' blocks per lane)
    const bool pair_layout = col_stride ? col_stride % 8 == 0 && (chunk_len / (uint32_t)D) % 8 == 0 && cm_reach
                                        : blk_bytes % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0;
    // (a float source takes it whatever SPRINTZ_OPT_ENC_PAIR says: nothing else serves its small batches fast)
    if ((flt || (k.enc_pair > 0 && nchunks >= (uint64_t)k.enc_pair)) && fast_common && D >= 5 && pair_layout && (uint64_t)chunk_len * esz >= 2 * blk_bytes) {
        int pdp = 4;
        while (2 * pdp < D) pdp <<= 1;
        const size_t pgroups = kThreads / pdp;
        // the window as long as it must be (the linear window needs no power of two): 592 instead of 672 bytes a chunk at 8 uint16 columns,
        // four workgroups a CU instead of three
        p.cap = ((uint32_t)group_bytes_max(esz, D) + 48u + (uint32_t)(SPRINTZ_ENC_DRAIN_ALIGN - 16) + 15u) & ~15u;
        // input staging: one 8 x D block (row-major: LDS transpose) or a burst of 4 blocks x (2 * pdp) columns (column-major)
        const size_t pstage = col_stride ? (size_t)4 * (2 * pdp) * (esz == 2 ? 16 : 8) : ((blk_bytes + 15) & ~(size_t)15);
        p.lds_group_stride = (uint32_t)(p.cap + pstage + 16);
        if ((p.lds_group_stride / 16) % 2 == 0) p.lds_group_stride += 16;    // an odd number of 16-byte units: the chunks of a wavefront start on different banks
        p.dp = pdp;
        p.exact = D == 2 * pdp;
        p.fused = fuses(pgroups);
        return plan_take(p, SPRINTZ_KF_ENC_PAIR, (nchunks * (uint64_t)pdp + kThreads - 1) / kThreads, (uint64_t)p.lds_group_stride * pgroups + qtab);
    }
    if (fast && !flt) {
        const size_t fgroups = kThreads / fdp;
        p.cap = cap_drain;
        // input staging: one 8 x D block (row-major: LDS transpose) or two bursts of 4 blocks x fdp columns (column-major)
        const size_t in_stage = col_stride ? (size_t)4 * fdp * (esz == 2 ? 16 : 8) : ((blk_bytes + 15) & ~(size_t)15);
        p.lds_group_stride = (uint32_t)(p.cap + in_stage + 16);
        p.dp = fdp;
        p.exact = D == fdp;
        p.fused = fuses(fgroups);
        return plan_take(p, SPRINTZ_KF_ENC_FAST, (nchunks * (uint64_t)fdp + kThreads - 1) / kThreads, (uint64_t)p.lds_group_stride * fgroups);
    }
    // streams of 65 .. 128 columns (BASELINE config 3): two columns per lane (encode_wide.h)
    if (!lowdim && !p.raw && !col_stride && D > 64 && D <= 128 && blk_bytes % 16 == 0 && ((uint64_t)chunk_len * esz) % 16 == 0 &&
        (uint64_t)chunk_len * esz >= 2 * blk_bytes && (s.src_lo % 16) == 0 && !k.no_fast) {
        // (8 bits, 65 .. 80 columns: 32 lanes a chunk -- a pair + a single column per lane -- two chunks a wavefront)
        const bool wsplit = esz == 1 && D <= 80 && k.split_lanes != 0;
        const size_t wlanes = wsplit ? 32 : 64, wgroups = kThreads / wlanes;
        p.cap = cap_drain;
        p.lds_group_stride = (uint32_t)(p.cap + ((blk_bytes + 15) & ~(size_t)15) + 16);
        p.dp = (int)wlanes;
        p.exact = D == 128;
        p.fused = fuses(wgroups);
        return plan_take(p, wsplit ? SPRINTZ_KF_ENC_SPLIT : SPRINTZ_KF_ENC_WIDE, (nchunks * (uint64_t)wlanes + kThreads - 1) / kThreads, (uint64_t)p.lds_group_stride * wgroups + qtab);
    }
    // univariate streams: one lane per chunk, quad-loaded 64-byte input windows, 64-byte output units (encode_uni.h)
    // (and the other low-dim shapes: 2 columns, 3 and 4 at 8 bits)
    // (round 6: the container inside THIS launch was built too -- 256 chunks a workgroup, 2 048 workgroups on BASELINE config 1, a short chain --
    //  and measured: 0.405 ms with a lane-parallel copy (a piece's chunk found by bisection), 0.49 - 0.51 chunk by chunk, against 0.3945 for
    //  encode + scan + copy in a row: streams of ~440 bytes re-read from their slots cost the workgroup what the copy pass costs.  Not kept.)
    if (!flt && lowdim && (D <= 2 || esz == 1) && !col_stride && !k.no_fast) return plan_take(p, SPRINTZ_KF_ENC_UNI, (nchunks + 255) / 256, 0);
    return plan_take(p, SPRINTZ_KF_ENC_GENERIC, (nchunks * (uint64_t)DP + kThreads - 1) / kThreads, shmem);
}

// compress_batch_dense: how the 16-byte aligned container is built.  DENSE_VERBATIM: chunks too short for a group -- all of them verbatim,
// all sizes known -- written straight into the container (api.hip: verbatim_dense_kernel); otherwise *enc is the encoder's plan, with the
// container inside its launch (DENSE_FUSED) or behind it by the scan + copy passes (DENSE_COMPACT: low-dim, more than 64 columns,
// misaligned blocks, SPRINTZ_OPT_DENSE_MODE 0).
// (Tried and dropped, measured on the headline batch: the batch in 4 parts, a part's scan + copy on a second stream while
//  the next part encodes -- 0.87 ms against 0.79 for the launches in a row; the kernels do not fill each other's gaps.)
inline Plan plan_dense(const Shape& s, const Knobs& k, Plan* enc)
{
    Plan p;
    // (never for a float source: the verbatim kernel copies raw source bytes -- such chunks go through the encoder's own tail)
    if (s.q != kQueryFloat && k.dense_mode && (s.codec == SPRINTZ_CODEC_DELTA || s.codec == SPRINTZ_CODEC_XFF) && !is_lowdim(s.esz, s.D) &&
        (s.chunk_len < 128u || s.chunk_len < 16u * (uint32_t)s.D) && s.chunk_len <= 0xffffu)
        return plan_take(p, SPRINTZ_KF_DENSE_VERBATIM, (s.nchunks * 64 + kThreads - 1) / kThreads, 0);
    Shape se = s;
    se.dense = k.dense_mode != 0;
    *enc = plan_encode(se, k);
    if (enc->err) return plan_fail(p, enc->err, enc->what);
    p.family = enc->fused ? SPRINTZ_KF_DENSE_FUSED : SPRINTZ_KF_DENSE_COMPACT;
    return p;
}

}  // namespace sprintz
