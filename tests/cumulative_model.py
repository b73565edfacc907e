"""The specification of cumulative rows (sprintz_mi355x_cumulative_rows, ChunkedCodec.cumulative_rows), in numpy.

A batch of n elements, chunk_len a multiple of D, is ONE sequence of batch rows g = 0 .. G - 1, G = ceil(n / D): row g is row g % R of
chunk g // R, R = chunk_len / D, and since rows do not straddle chunks element e of the flat input sits in row e // D and column e % D.
A partial last row has the columns it has.  For every element that exists

    min[g, d] = min(seed_min[d], x[0 .. g, d])        unsigned, in the element type
    max[g, d] = max(seed_max[d], x[0 .. g, d])        unsigned, in the element type
    sum[g, d] = seed_sum[d] + sum(x[0 .. g, d])       modulo 2^64

The seeds are a carry, uint64 [3, D]: a min row, a max row (both read modulo 2^(8 esz)) and a sum row; None is the identities -- all
ones of the element type, 0 and 0.  The state behind the batch's last element of each column is the carry the call hands out: given to
the next call it yields the cumulative of the concatenated batches.  The row of an op that was not asked for is its seed, passed through.
A damaged chunk contributes the identity to everything behind it and to the carry; what its own elements get is not specified.
The results are flat arrays of n elements, element e at place e -- where decompress_batch places the element itself; the sum is kept as
uint64 (int64() and low32() give the two forms the library stores)."""
import numpy as np

import rolling_model as rm

MIN, MAX, SUM = 1, 2, 4
OPS = {"min": MIN, "max": MAX, "sum": SUM}
SUBSETS = (1, 2, 4, 3, 5, 6, 7)                          # every non-empty subset of the ops, as the C-ABI's mask
M64 = (1 << 64) - 1


def names(mask):
    return tuple(k for k, bit in OPS.items() if mask & bit)


def identity(D, esz):
    """the carry in front of a stream's first batch"""
    c = np.zeros((3, D), np.uint64)
    c[0] = (1 << (8 * esz)) - 1
    return c


def seeds(carry, D, esz):
    """a carry as the library reads it: the min and the max rows modulo 2^(8 esz)"""
    c = identity(D, esz) if carry is None else np.array(carry, dtype=np.uint64).reshape(3, D)
    c[:2] &= np.uint64((1 << (8 * esz)) - 1)
    return c


def cumulative(x, D, carry=None, ops=7, chunk_len=None, bad=()):
    """x: the batch's n elements, flat -> ({"min", "max": x's dtype [n], "sum": uint64 [n]} of the ops asked for, carry uint64 [3, D]).
    bad: the damaged chunks (of chunk_len elements each), whose elements count as absent"""
    n, esz = x.size, x.dtype.itemsize
    G = -(-n // D)
    top = (1 << (8 * esz)) - 1
    seed = seeds(carry, D, esz)
    there = np.zeros(G * D, bool)
    there[:n] = True
    for c in bad:
        there[c * chunk_len:(c + 1) * chunk_len] = False
    there = there.reshape(G, D)
    m = np.zeros(G * D, np.uint64)
    m[:n] = x
    m = m.reshape(G, D)
    out, left = {}, seed.copy()
    if ops & MIN:
        r = np.minimum(np.minimum.accumulate(np.where(there, m, np.uint64(top)), axis=0), seed[0][None, :]) if G else m
        out["min"] = r.reshape(-1)[:n].astype(x.dtype)
        if G:
            left[0] = r[-1]
    if ops & MAX:
        r = np.maximum(np.maximum.accumulate(np.where(there, m, np.uint64(0)), axis=0), seed[1][None, :]) if G else m
        out["max"] = r.reshape(-1)[:n].astype(x.dtype)
        if G:
            left[1] = r[-1]
    if ops & SUM:
        r = np.cumsum(np.where(there, m, np.uint64(0)), axis=0, dtype=np.uint64) + seed[2][None, :] if G else m       # (uint64 arrays wrap modulo 2^64)
        out["sum"] = r.reshape(-1)[:n].astype(np.uint64)
        if G:
            left[2] = r[-1]
    return out, left


def int64(total):
    """the uint64 sums as the library stores them with sum_bytes 8"""
    return total.view(np.int64)


def low32(total):
    """... and with sum_bytes 4: the low half"""
    return (total & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def mean(total, D, rows_before=0):
    """flat uint64 sums of n elements -> float64 expanding means, flat: the int64 sum over the rows so far"""
    g = np.arange(total.size) // D
    return int64(total).astype(np.float64) / (rows_before + g + 1).astype(np.float64)


def brute(x, D, carry=None):
    """the definition, element by element, in Python's integers"""
    esz = x.dtype.itemsize
    seed = seeds(carry, D, esz)
    mn, mx, sm = [int(v) for v in seed[0]], [int(v) for v in seed[1]], [int(v) for v in seed[2]]
    out = {"min": np.zeros(x.size, x.dtype), "max": np.zeros(x.size, x.dtype), "sum": np.zeros(x.size, np.uint64)}
    for e in range(x.size):
        d, v = e % D, int(x[e])
        mn[d], mx[d], sm[d] = min(mn[d], v), max(mx[d], v), (sm[d] + v) & M64
        out["min"][e], out["max"][e], out["sum"][e] = mn[d], mx[d], sm[d]
    return out, np.array([mn, mx, sm], dtype=np.uint64)


def chained(x, D, cuts, carry=None, ops=7):
    """the batch cut at the rows `cuts` (ascending row numbers) into batches of their own, each seeded with the carry of the one in front"""
    parts, lo = [], 0
    for hi in list(cuts) + [-(-x.size // D)]:
        got, carry = cumulative(x[lo * D:hi * D], D, carry, ops)
        parts.append(got)
        lo = hi
    return {k: np.concatenate([p[k] for p in parts]) for k in names(ops)}, carry


# ---- geom.h's formulas, restated: the scan's tile and the call's scratch

THREADS = 256
SCAN_CHUNKS = 8                                          # kCumScanChunks: consecutive chunks a thread of the scan takes
SCAN_TILE = THREADS * SCAN_CHUNKS                        # kCumScanTile: chunks a workgroup of the scan takes at a step


def r16(v):
    return (v + 15) & ~15


def tmp_layout(nchunks, D):
    """cum_tmp_layout: the byte offsets of the states, the totals pass' return values, its sums, minima and maxima, and the whole size"""
    nd = nchunks * D
    rets = r16(nd * 24)
    total = rets + r16(nchunks * 8)
    mn = total + r16(nd * 8)
    mx = mn + r16(nd * 2)
    return dict(state=0, rets=rets, sum=total, min=mn, max=mx, bytes=mx + r16(nd * 2))


def tmp_bytes(nchunks, D):
    return tmp_layout(nchunks, D)["bytes"] if nchunks > 1 else 0


# ---- plan.h's cumulative branch, restated (rolling_model restates decode_fast_map and choose_mapping)

def out_esz(esz, ops, sum_bytes):
    """the widest output element of a call"""
    return sum_bytes if ops & SUM else esz


def fast_takes(esz, D, chunk_len, general=False, no_fast=False, out_lo=0, out_esz=8):
    """does decode_fast.h serve the call: rows of whole 16-byte pieces on a one-column-a-lane mapping, aligned outputs, within the
    descriptors' reach in output bytes"""
    lowdim = not general and D <= (4 if esz == 1 else 2)
    dp, cpl, carve = rm.fast_map(esz, D)
    return (not lowdim and not no_fast and cpl == 1 and 2 * D > dp and chunk_len * esz * 2 >= carve and (D * esz) % 16 == 0 and
            (chunk_len * esz) % 16 == 0 and out_lo % 16 == 0 and chunk_len * out_esz * 4096 < 0xf0000000)
