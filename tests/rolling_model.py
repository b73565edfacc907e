"""The specification of rolling rows (sprintz_mi355x_rolling_rows, ChunkedCodec.rolling_rows), in numpy.

A batch of n elements, chunk_len a multiple of D, is ONE sequence of batch rows g = 0 .. G - 1, G = ceil(n / D): row g is row g % R of
chunk g // R, R = chunk_len / D, and since rows do not straddle chunks element e of the flat input sits in row e // D and column e % D.
A partial last row has the columns it has.  For every element that exists

    out[g, d] = op(x[max(0, g - W + 1) .. g, d])

a trailing window of W rows, clipped at the batch's first row (pandas' rolling(W, min_periods=1)): min and max in the element type,
unsigned; sum as an int32 (W * (2^(8 esz) - 1) < 2^31: it is exact); mean = float32(sum) / float32(min(g + 1, W)), one float32 divide.
The results are flat arrays of n elements, element e at place e -- where decompress_batch places the element itself."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MIN, MAX, SUM = 1, 2, 4
OPS = {"min": MIN, "max": MAX, "sum": SUM}
SUBSETS = (1, 2, 4, 3, 5, 6, 7)                          # every non-empty subset of the ops, as the C-ABI's mask


def names(mask):
    return tuple(k for k, bit in OPS.items() if mask & bit)


def check_window(W, R, esz):
    """the rules of W: a multiple of 8, 8 <= W <= R, and a sum that fits int32"""
    return W >= 8 and W % 8 == 0 and W <= R and W * ((1 << (8 * esz)) - 1) < (1 << 31)


def counts(G, W):
    """the rows in the window that ends at batch row g"""
    return np.minimum(np.arange(G, dtype=np.int64) + 1, W)


def rolling(x, D, W):
    """x: the batch's n elements, flat -> {"min", "max": x's dtype [n], "sum": int32 [n]}"""
    n = x.size
    G = -(-n // D)
    top = (1 << (8 * x.dtype.itemsize)) - 1
    m = np.zeros(G * D, np.int64)
    m[:n] = x
    m = m.reshape(G, D)                                   # (the columns a partial last row lacks: cut off below, and no window behind them)
    out = {}
    for name, pad, red in (("min", top, np.min), ("max", 0, np.max), ("sum", 0, np.sum)):
        padded = np.concatenate([np.full((W - 1, D), pad, np.int64), m])          # front-padded with the op's identity: the clipped windows
        r = red(sliding_window_view(padded, W, axis=0), axis=-1)                  # [G, D]: window g ends at row g
        out[name] = r.reshape(-1)[:n].astype(np.int32 if name == "sum" else x.dtype)
    return out


def rolling_local(x, chunk_len, D, W):
    """the same with every chunk its own beginning: what the decode launch leaves before the seam pass, and what stays behind a damaged chunk"""
    parts = [rolling(x[lo:lo + chunk_len], D, W) for lo in range(0, x.size, chunk_len)]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("min", "max", "sum")}


def mean(total, D, W):
    """flat int32 sums of n elements -> float32 means, flat"""
    g = np.arange(total.size) // D
    return total.astype(np.float32) / np.minimum(g + 1, W).astype(np.float32)


def brute(x, D, W):
    """the definition, element by element"""
    out = {"min": np.zeros(x.size, x.dtype), "max": np.zeros(x.size, x.dtype), "sum": np.zeros(x.size, np.int32)}
    for e in range(x.size):
        win = x[max(e % D, e - (W - 1) * D):e + 1:D].astype(np.int64)
        out["min"][e], out["max"][e], out["sum"][e] = win.min(), win.max(), win.sum()
    return out


# ---- geom.h's formulas, restated: the history ring of a chunk, the largest window a shape takes, the seam scratch

THREADS = 256
LDS_MAX = 160 * 1024
CPL_SET = (1, 2, 3, 4, 5, 6, 8)


def lanes(esz, D, general):
    """choose_mapping: the lanes of the generic kernel's column group"""
    if not general and D <= (4 if esz == 1 else 2):
        return 1 << max(D - 1, 0).bit_length()
    fits = [(l, c) for l in range(7) for c in CPL_SET if (1 << l) * c >= D]
    best = max(D / ((1 << l) * c) for l, c in fits)
    for l in range(6, -1, -1):
        for c in CPL_SET:
            if (1 << l) * c >= D and D / ((1 << l) * c) >= 0.75 * best:
                return 1 << l
    return 64


def ring_bytes(W, D, esz):
    return ((W + 8) * D * esz + 15) & ~15


def sum_max_window(esz):
    return ((1 << 31) - 1) // ((1 << (8 * esz)) - 1) & ~7


def max_window(esz, D, general):
    """the largest W whose rings -- one for each of a workgroup's chunks -- fit 160 KB, and whose sum fits int32"""
    groups = THREADS // lanes(esz, D, general)
    rows = (LDS_MAX // groups & ~15) // (D * esz)
    w = 0 if rows < 16 else (rows - 8) & ~7
    return min(w, sum_max_window(esz))


def tmp_stride(W, D, esz):
    return (16 + (W - 1) * D * esz + 15) & ~15


# ---- decode_fast.h's side, restated from geom.h (decode_fast_lds_bytes) and plan.h (decode_fast_map, the rolling branch of plan_decode)

FAST_LDS_BUDGET = 80 * 1024


def fast_map(esz, D):
    """-> (lanes a chunk, columns a lane, LDS bytes of one group's carve)"""
    dp, cpl = 4, 1
    while dp < D and dp < 64:
        dp <<= 1
    while dp * cpl < D:
        cpl <<= 1
    W = 8 * esz
    unit, hb, dcap = dp * 16 * cpl, (3 if W == 8 else 4), dp * cpl
    hdrmax, blkmax = (2 * dcap * hb + 7) // 8, 8 * dcap * esz
    cg = hdrmax + 2 * blkmax + 4
    rb = ((2 * (cg + 24) + 3 + unit - 1) // unit + 1) * unit
    apron = (cg + 24 + 8 + 15) & ~15
    stage = ((8 * D * esz + 15) & ~15) + 16
    return dp, cpl, rb + apron + stage


def fast_takes(esz, D, chunk_len, W, general=False, no_fast=False, out_lo=0, out_esz=4):
    """does decode_fast.h serve the call: rows of whole 16-byte pieces on a one-column-a-lane mapping, aligned outputs, within the descriptors'
    reach in output bytes, and both rings of every group of a workgroup inside the budget"""
    lowdim = not general and D <= (4 if esz == 1 else 2)
    dp, cpl, carve = fast_map(esz, D)
    return (not lowdim and not no_fast and cpl == 1 and 2 * D > dp and chunk_len * esz * 2 >= carve and (D * esz) % 16 == 0 and
            (chunk_len * esz) % 16 == 0 and out_lo % 16 == 0 and chunk_len * out_esz * 4096 < 0xf0000000 and
            (carve + ring_bytes(W, D, esz)) * (THREADS // dp) <= FAST_LDS_BUDGET)


def fast_max_window(esz, D):
    """the largest W (a multiple of 8; 0: none) at which the two rings of a workgroup's groups fit the budget"""
    dp, cpl, carve = fast_map(esz, D)
    rows = ((FAST_LDS_BUDGET // (THREADS // dp) - carve) & ~15) // (D * esz)
    return 0 if rows < 16 else (rows - 8) & ~7
