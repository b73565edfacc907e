// transform_plan.h -- how the stand-alone delta / double-delta DECODE (transforms.hip) serves a stream: which of its three forms, cut into
// which pieces, with which runs, levels and tiles, and WHERE in d_tmp every array of the call lies.  One pure function of the shape, the low
// four bits of the two pointers, the SPRINTZ_MI355X_TRANSFORM_CHAIN setting and the CU count; no HIP, no pointer, no environment -- plain
// C++17 like plan.h, so that the CPU tests build it with a host compiler (tests/transform_plan_probe.cpp, tests/test_transform_plan_cpu.py).
//
// sprintz_mi355x_transform_tmp_bytes and the launcher both read THIS description: the size is the largest `used` over every form a caller's
// pointers and setting can select, so it cannot price one layout while the launcher places another.  (It did: the size counted one summary
// per 16 rows -- the generic levels' layout -- while the wave scan places one per RUN, and a run of one load of rows with 22 .. 64 pieces
// is 4 .. 8 rows: level 1 took 2 .. 4 times what was counted.  The chain's slack, 8 KiB + len / 8, hid it below ~7 KB of stream.)
//
// Every predicate keeps the terms and the order it had at the launch sites: no shape changes its form, piece, run length or grid here.
#pragma once

#include "../../include/sprintz_mi355x.h"

// experiment builds' switches (tools/build_variant.sh): the constants below are what the kernels are compiled with
#ifndef TR_RUN_LOADS
#define TR_RUN_LOADS 16
#endif
#ifndef TR_CHAIN_LOADS
#define TR_CHAIN_LOADS 4
#endif
#ifndef TR_CHAIN_WAVES
#define TR_CHAIN_WAVES 8
#endif
#ifndef TR_CHAIN_WGS_PER_CU
#define TR_CHAIN_WGS_PER_CU 1
#endif
#ifndef TR_CHAIN_MIN_TILES
#define TR_CHAIN_MIN_TILES 1                  // (from the first tile on: 9.6 against 13.7 us at 32 KB, 13 against 52 at 0.5 MB, 64 against 90 at 128 MB -- tools/chain_sizes.py)
#endif

namespace sprintz {

constexpr int kTrR = 16;                      // rows (or lower-level runs) folded by one thread of the generic levels
constexpr int kTrTB = 256;
constexpr int kTrTopT = 1024;                 // threads of scan_runs_kernel's one workgroup
constexpr int kTrRunLoads = TR_RUN_LOADS;     // loads a run of the wave scan, at most
constexpr int kTrRowsPerLane = 4;
constexpr int kTrChainWaves = TR_CHAIN_WAVES, kTrChainLoads = TR_CHAIN_LOADS, kTrChainMaxDv = 8;
constexpr int kTrMaxLevels = 12;              // len < 2^37 (check()): at most 10 levels of 16 above the rows, one more for the runs
constexpr uint64_t kTrNone = ~0ull;           // an array the call does not have (s2 / din of delta)
constexpr uint64_t kTrChainNever = ~0ull;     // chain_min of SPRINTZ_MI355X_TRANSFORM_CHAIN=0

enum { kTrTopNone = 0, kTrTopRuns = 1, kTrTopLevels = 2 };

struct TrShape {
    int kind = 0, esz = 1;                    // 0 delta, 1 double delta; element bytes
    uint64_t len = 0;                         // elements
    uint32_t D = 1;                           // ndims
    unsigned src_lo = 0, dst_lo = 0;          // the low four bits of the source and destination addresses
    uint64_t chain_min = TR_CHAIN_MIN_TILES;  // the one-pass decode from this many tiles on (kTrChainNever: never)
    uint32_t cus = 256;                       // workgroups of the one-pass decode that are resident at once
};

// one level of summaries: `rows` runs of `span` original rows, four (double delta) or two arrays of `bytes` each at these offsets of d_tmp
// (the generic levels' top level, rows == 1: none)
struct TrLevel {
    uint64_t rows = 0, span = 0, bytes = 0;
    uint64_t s1 = kTrNone, s2 = kTrNone, xin = kTrNone, din = kTrNone;
};

struct TrPlan {
    int family = -1;                          // SPRINTZ_KF_TR_CHAIN / _TR_WAVE / _TR_LEVELS
    int piece = 0;                            // bytes of a piece: 16, 4, 2 or 1 (0: the generic levels alone)
    int M = 1;                                // rows inside a piece (Sub<P, RB>: rows of 1 / 2 / 4 / 8 bytes)
    uint32_t D = 0;                           // elements of a row as the levels see it (M > 1: the 16 / esz elements of a piece)
    uint32_t dv = 0;                          // pieces a row
    uint64_t len_e = 0, rows0 = 0;            // pieces of the stream; its rows, a ragged last one counted
    int run_loads = 0;
    uint64_t run_rows = 0, nruns = 0, grid = 0;
    int top = kTrTopNone;                     // what hands the runs their incoming states
    uint32_t G = 0;                           // scan_runs_kernel: slices of the runs
    int nlevels = 0;                          // lv[0 .. nlevels): wave -- lv[0] is the runs' level, the generic levels above it behind; levels -- all generic
    TrLevel lv[kTrMaxLevels];
    // the one-pass decode: the ticket word, then arrays of `arr` bytes of tagged 64-bit words; the first `need` bytes are zeroed by the call
    uint64_t tile_e = 0, ntiles = 0, arr = 0, need = 0, wgs = 0;
    uint64_t ticket = kTrNone, agg1 = kTrNone, inc1 = kTrNone, agg2 = kTrNone, inc2 = kTrNone;
    uint64_t used = 0;                        // bytes of d_tmp the call touches: [0, used)
};

// scratch of the one-pass decode: the ticket + two (delta) or four arrays of dv x 4 tagged 64-bit words per tile.  A tile is 8 waves x 4
// loads x >= 56 pieces x 4 rows, dv <= 8: about 1 % of the stream -- the bound is the rule that keeps the form, not the size reported
inline uint64_t tr_chain_bound(uint64_t stream_bytes) { return stream_bytes / 8 + 8192; }

// the levels above a base of `rows` runs of `span` rows, placed from byte `t` of d_tmp on; returns the first byte behind them.
// The top level -- a single run, entering with the zero state -- has no arrays: nothing reads its summary and nothing hands it a state, so
// it is neither reduced into nor placed (it used to be: one row of ndims elements four times over, 4 x the stream at 65 535 columns x 2 rows)
inline uint64_t tr_levels(TrPlan& p, int kind, int esz, uint64_t rows, uint64_t span, uint64_t t)
{
    while (rows > 1 && p.nlevels < kTrMaxLevels) {       // the top level is a single run
        rows = (rows + kTrR - 1) / kTrR;
        span *= kTrR;
        TrLevel& l = p.lv[p.nlevels++];
        l.rows = rows;
        l.span = span;
        if (rows == 1) break;
        l.bytes = (rows * p.D * (uint64_t)esz + 63) & ~(uint64_t)63;
        l.s1 = t; t += l.bytes;
        if (kind) { l.s2 = t; t += l.bytes; }
        l.xin = t; t += l.bytes;
        if (kind) { l.din = t; t += l.bytes; }
    }
    return t;
}

// piece size of the wave-scan path: 16, 4 or one element's bytes -- the largest that divides the row, the stream and the pointers'
// alignment, with at most 64 pieces a row
inline int tr_wave_piece_bytes(int esz, uint64_t len, uint32_t D, unsigned ptr_lo)
{
    const uint64_t row_bytes = (uint64_t)D * esz, total = len * esz;
    const int sizes[3] = {16, 4, esz};
    for (int pb : sizes) {
        if (pb < esz || row_bytes % pb || total % pb) continue;
        if (ptr_lo % pb) continue;
        const uint64_t dv = row_bytes / pb;
        // any piece count up to 64 (64 / dv whole rows per load); 1 and 2 go through the LDS hand-over, which is laid out for 64 pieces
        if (dv <= 64 && ((dv & (dv - 1)) == 0 || dv >= 3)) return pb;
    }
    return 0;
}

inline TrPlan tr_plan(const TrShape& s)
{
    TrPlan p;
    const int esz = s.esz, kind = s.kind;
    const uint64_t len = s.len, rb = (uint64_t)s.D * esz;
    const unsigned ptr_lo = (s.src_lo | s.dst_lo) & 15u;
    p.rows0 = (len + s.D - 1) / s.D;
    p.D = s.D;
    if (rb < 16 && 16 % rb == 0 && (len * esz) % 16 == 0 && ptr_lo % 16 == 0) {       // rows shorter than a piece
        p.piece = 16;
        p.M = (int)(16 / rb);
    } else {
        p.piece = tr_wave_piece_bytes(esz, len, s.D, ptr_lo);
    }
    if (!p.piece) {                                      // the generic levels alone: level 0 is the input itself
        p.family = SPRINTZ_KF_TR_LEVELS;
        p.used = tr_levels(p, kind, esz, p.rows0, 1, 0);
        return p;
    }
    // (rows shorter than a piece: the levels above see the replicated 16-byte pieces as rows of 16 / esz columns)
    if (p.M > 1) p.D = (uint32_t)(16 / esz);
    p.dv = p.M > 1 ? 1u : (uint32_t)(rb / (uint64_t)p.piece);
    const uint32_t dv = p.dv;
    p.len_e = len * esz / (uint64_t)p.piece;
    // loads a run: 16 where there are runs enough to fill the chip; short streams take 4 or 1 -- a run's loads are a serial chain, and a stream of
    // eight 16-load runs was two passes of 16 dependent round trips on eight waves: 52 us for 0.5 MB (tools/chain_sizes.py) -- as long as the
    // runs' states still come from the one workgroup of scan_runs_kernel (<= 4 096 runs)
    p.run_loads = kTrRunLoads;
    {
        const uint64_t rows16 = (uint64_t)kTrRunLoads * kTrRowsPerLane * (64 / dv) * p.M, n16 = (p.rows0 + rows16 - 1) / rows16;
        if (n16 * 16 <= 4096) p.run_loads = 1;
        else if (n16 * 4 <= 4096) p.run_loads = 4;
    }
    p.run_rows = (uint64_t)p.run_loads * kTrRowsPerLane * (64 / dv) * p.M;
    p.nruns = (p.rows0 + p.run_rows - 1) / p.run_rows;
    p.grid = (p.nruns * 64 + kTrTB - 1) / kTrTB;
    // ---- streams of at least chain_min tiles, rows of at most kTrChainMaxDv pieces: one pass (chain_scan_kernel)
    // (16-bit elements only: at 8 bits the packed arithmetic is five instructions an add where v_pk_add_u16 is one, the tile's fold and walk
    //  run on one workgroup a CU, and the form measured SLOWER than the two passes on every column count -- tools/transforms_shapes.py:
    //  delta 0.126 - 0.167 against 0.103 - 0.143 ms on 128 MiB, double delta 0.28 - 0.48 against 0.15 - 0.26; at 16 bits 0.063 - 0.074 against 0.090 - 0.124.
    //  And 16-byte pieces only: with 4- or 2-byte pieces (rows that are not multiples of 16 bytes) a tile is 32 / 16 KB and the look-back is the kernel:
    //  3 / 5 / 7 / 10 / 12 uint16 columns 0.199 / 0.284 / 0.220 / 0.147 / 0.133 against 0.160 / 0.158 / 0.154 / 0.125 / 0.121 ms.)
    if (esz == 2 && p.piece == 16 && dv <= (uint32_t)kTrChainMaxDv) {
        const uint64_t tile_e = (uint64_t)kTrChainWaves * kTrChainLoads * (uint64_t)((64 / dv) * dv) * kTrRowsPerLane;
        const uint64_t ntiles = (p.len_e + tile_e - 1) / tile_e;
        const uint64_t arr = (ntiles * dv * 4 * 8 + 255) & ~(uint64_t)255, need = 256 + (kind ? 4 : 2) * arr;      // 4 tagged words a 16-byte piece
        p.tile_e = tile_e;
        if (ntiles >= s.chain_min && ntiles < 0x7fffffffull && need <= tr_chain_bound(len * esz)) {
            p.family = SPRINTZ_KF_TR_CHAIN;
            p.ntiles = ntiles; p.arr = arr; p.need = need;
            p.wgs = ntiles < (uint64_t)s.cus ? ntiles : (uint64_t)s.cus;
            p.ticket = 0;
            p.agg1 = 256;
            p.inc1 = 256 + arr;
            if (kind) { p.agg2 = 256 + 2 * arr; p.inc2 = 256 + 3 * arr; }
            p.used = need;
            return p;
        }
    }
    p.family = SPRINTZ_KF_TR_WAVE;
    if (p.nruns == 1) return p;                          // one run: it enters with the zero state, no scratch
    // level 1 = one summary per run, laid out like rows of the stream
    TrLevel& l = p.lv[p.nlevels++];
    l.rows = p.nruns;
    l.span = p.run_rows;
    l.bytes = (p.nruns * p.D * (uint64_t)esz + 63) & ~(uint64_t)63;
    uint64_t t = 0;
    l.s1 = t; t += l.bytes;
    if (kind) { l.s2 = t; t += l.bytes; }
    l.xin = t; t += l.bytes;
    if (kind) { l.din = t; t += l.bytes; }
    if (p.D <= 64 && p.nruns <= 4096) {                  // (wide rows, or streams long enough that six ~4.6 us launches do not matter: the generic levels --
                                                         //  with 16 384 runs the one workgroup measured slower than they are: 0.72 against 0.66 ms at 512 Mi samples)
        const uint32_t Gmax = (uint32_t)kTrTopT / p.D;
        p.top = kTrTopRuns;
        p.G = (uint32_t)(p.nruns < Gmax ? p.nruns : Gmax);
    } else {
        p.top = kTrTopLevels;
        t = tr_levels(p, kind, esz, p.nruns, p.run_rows, t);
    }
    p.used = t;
    return p;
}

// every array of the call in d_tmp: f(name, byte offset, bytes).  All of them are live together.
template <typename F> inline void tr_arrays(const TrPlan& p, F f)
{
    if (p.family == SPRINTZ_KF_TR_CHAIN) {
        f("ticket", p.ticket, (uint64_t)256);
        f("agg1", p.agg1, p.arr);
        f("inc1", p.inc1, p.arr);
        if (p.agg2 != kTrNone) f("agg2", p.agg2, p.arr);
        if (p.inc2 != kTrNone) f("inc2", p.inc2, p.arr);
        return;
    }
    for (int k = 0; k < p.nlevels; k++) {
        const TrLevel& l = p.lv[k];
        if (l.s1 == kTrNone) continue;                   // the top level of the generic levels: no arrays
        f("s1", l.s1, l.bytes);
        if (l.s2 != kTrNone) f("s2", l.s2, l.bytes);
        f("xin", l.xin, l.bytes);
        if (l.din != kTrNone) f("din", l.din, l.bytes);
    }
}

// sprintz_mi355x_transform_tmp_bytes for delta / double delta: a caller sizes d_tmp before it knows where its buffers lie or what
// SPRINTZ_MI355X_TRANSFORM_CHAIN says, so this is the most that any of the forms those can select takes.  The pointers decide through
// (src | dest) % 16, % 4 and % esz alone -- four classes -- and the setting through "the one-pass decode or not"
inline uint64_t tr_tmp_bytes(int kind, int esz, uint64_t len, uint32_t D)
{
    uint64_t most = 0;
    const unsigned los[4] = {0u, 4u, 2u, 1u};
    const uint64_t chains[2] = {1, kTrChainNever};
    for (unsigned lo : los)
        for (uint64_t chain_min : chains) {
            TrShape s;
            s.kind = kind; s.esz = esz; s.len = len; s.D = D; s.src_lo = lo; s.chain_min = chain_min;
            const uint64_t used = tr_plan(s).used;
            if (used > most) most = used;
        }
    return ((most + 63) & ~(uint64_t)63) + 64;
}

}  // namespace sprintz
