"""The specification of FIR rows (sprintz_mi355x_fir_rows, ChunkedCodec.fir_rows), in numpy.  Applied to the ORIGINAL input -- decode is lossless
and pinned elsewhere.

A batch of n elements, chunk_len a multiple of D, is ONE sequence of batch rows g = 0 .. G - 1, G = ceil(n / D): row g is row g % R of chunk
g // R, R = chunk_len / D, and element e of the flat input sits in row e // D and column e % D.  A partial last row has the columns it has.  For
T taps, 1 <= T <= 256 with T - 1 <= R, and every element that exists, with x the unsigned element:

    y[g, d] = bias[d] + sum_{j = 0 .. T - 1} taps[j][d] x[g - j, d]          modulo 2^32, read as int32          (taps[0] weighs the row itself)

Rows in front of row 0 come from prev -- [T - 1, D], the last rows of the batch before this one, its last row being row -1 -- or, without prev,
equal row 0 (edge replication).  Accumulation is in int64 on values reduced modulo 2^32, so the wrap is the kernels'.  The float formats convert y
as derive rows convert a sum (derive_model.convert, with the scale and offset of the element's COLUMN).  The results are flat arrays of n
elements, element e at place e -- where decompress_batch places the element itself; floats are returned as BITS."""
import numpy as np

import derive_model as dm
import rolling_model as rm

I32 = dm.I32
FORMATS = dm.FORMATS
C_FORMAT = dm.C_FORMAT
OUT_BYTES = dm.OUT_BYTES
MAX_TAPS = 256


def wrap32(v):
    return (np.asarray(v, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def as_taps(taps, D):
    """[T] (shared by all columns) or [T, D] -> int64 [T, D]"""
    t = np.asarray(taps, np.int64)
    return np.repeat(t[:, None], D, axis=1) if t.ndim == 1 else t.reshape(-1, D)


def history(x, D, T, prev=None):
    """the batch's rows [G, D] (the columns a partial last row lacks hold 0: cut off by the callers) with the T - 1 rows in front of row 0 on
    top: prev's, or row 0 replicated -> int64 [T - 1 + G, D]"""
    x = np.asarray(x).ravel()
    n = x.size
    G = -(-n // D)
    m = np.zeros(G * D, np.int64)
    m[:n] = x
    m = m.reshape(G, D)
    if prev is not None:
        front = np.asarray(prev).astype(np.int64).reshape(T - 1, D)
    else:
        front = np.repeat(m[:1], T - 1, axis=0) if G else np.zeros((T - 1, D), np.int64)
    return np.concatenate([front, m])


def sums(x, D, taps, bias=None, prev=None):
    """y of every element of the flat batch x -> int64 [n], each value in int32's range"""
    x = np.asarray(x).ravel()
    t = as_taps(taps, D)
    T = t.shape[0]
    b = np.zeros(D, np.int64) if bias is None else np.broadcast_to(np.asarray(bias, np.int64), (D,))
    h = history(x, D, T, prev)
    G = h.shape[0] - (T - 1)
    y = np.broadcast_to(b, (G, D)).astype(np.int64)
    for j in range(T):
        y = wrap32(y + wrap32(t[j][None, :] * h[T - 1 - j:T - 1 - j + G]))       # (|tap| < 2^31 and x < 2^16: the product fits int64)
    return y.reshape(-1)[:x.size]


def sums_brute(x, D, taps, bias=None, prev=None):
    """the same definition, an element at a time, in Python integers"""
    x = [int(e) for e in np.asarray(x).ravel()]
    t = as_taps(taps, D)
    T = t.shape[0]
    pv = None if prev is None else np.asarray(prev).astype(np.int64).reshape(T - 1, D)
    out = np.zeros(len(x), np.int64)
    for e in range(len(x)):
        g, d = divmod(e, D)
        s = 0 if bias is None else int(np.broadcast_to(np.asarray(bias, np.int64), (D,))[d])
        for j in range(T):
            r = g - j
            v = x[r * D + d] if r >= 0 else int(pv[T - 1 + r, d]) if pv is not None else x[d]
            s += int(t[j, d]) * v
        out[e] = (s + (1 << 31)) % (1 << 32) - (1 << 31)
    return out


def sums_local(x, chunk_len, D, taps, bias=None):
    """the chunk-local variant: every chunk its own beginning, the rows in front of its row 0 contributing NOTHING (zeros) -- what the decode
    launch leaves before the seam pass, and what stays in the first T - 1 rows of a chunk behind a damaged one"""
    t = as_taps(taps, D)
    zero = np.zeros((t.shape[0] - 1, D), np.int64)
    x = np.asarray(x).ravel()
    return np.concatenate([sums(x[lo:lo + chunk_len], D, t, bias, zero) for lo in range(0, x.size, chunk_len)])


def convert(y, D, fmt, scale=None, offset=None):
    """y int64 [n] -> the output's BITS [n]: element e takes the scale and offset of column e % D"""
    y = np.asarray(y, np.int64)
    if fmt == I32:
        return y.astype(np.int32).view(np.uint32)
    n = y.size
    G = -(-n // D)
    full = np.zeros(G * D, np.int64)
    full[:n] = y
    return dm.convert(full.reshape(G, D), fmt, scale, offset).reshape(-1)[:n]


def fir_rows(x, D, taps, bias=None, fmt=I32, scale=None, offset=None, prev=None):
    return convert(sums(x, D, taps, bias, prev), D, fmt, scale, offset)


def bound(esz, taps, bias, D):
    """per column |bias[d]| + (2^(8 esz) - 1) sum_j |taps[j][d]| -> int [D] (Python integers): below 2^31 the value is exact"""
    t = as_taps(taps, D)
    b = np.broadcast_to(np.asarray(0 if bias is None else bias, np.int64), (D,))
    top = (1 << (8 * esz)) - 1
    return [abs(int(b[d])) + top * sum(abs(int(v)) for v in t[:, d]) for d in range(D)]


def random_taps(rng, T, D, esz, exact=True):
    """random signed taps that differ per column and a bias, [T, D] and [D]: within the exactness bound, or (exact=False) anywhere in int32"""
    if not exact:
        return rng.integers(-(1 << 31), 1 << 31, (T, D)), rng.integers(-(1 << 31), 1 << 31, D)
    top = (1 << (8 * esz)) - 1
    tmax = max(1, ((1 << 31) - 1) // (top * T) - 1)
    t = rng.integers(-tmax, tmax + 1, (T, D))
    left = (1 << 31) - 1 - top * np.abs(t).sum(axis=0)
    return t, rng.integers(-left, left + 1)


def tail_rows(x, D, T, prev=None):
    """the last T - 1 whole rows of (the rows in front, then the batch): the prev of the next batch -> [T - 1, D] of x's dtype"""
    x = np.asarray(x).ravel()
    G = x.size // D
    h = history(x[:G * D], D, T, prev)
    return h[h.shape[0] - (T - 1):].astype(x.dtype)


# ---- geom.h's formulas, restated (the ring is rolling rows' with W replaced by Wh), and plan.h's FIR branch

def history_rows(T):
    """Wh: T - 1 rounded up to whole blocks of 8 rows"""
    return (T + 6) & ~7


def ring_bytes(T, D, esz):
    return rm.ring_bytes(history_rows(T), D, esz)


def tmp_stride(T, D, esz):
    """the seam scratch of one chunk: a 16-byte head, the first T - 1 rows, the last T - 1 rows, rounded up to 16"""
    return (16 + 2 * (T - 1) * D * esz + 15) & ~15


def max_taps(esz, D, general):
    """the most taps whose rings -- one for each of a workgroup's chunks -- fit 160 KB"""
    groups = rm.THREADS // rm.lanes(esz, D, general)
    rows = (rm.LDS_MAX // groups & ~15) // (D * esz)
    return 0 if rows < 8 else min(((rows - 8) & ~7) + 1, MAX_TAPS)


def fast_lds(esz, D, T):
    """decode_fast.h's launch LDS in this mode: the groups' carves, a ring a group behind them, the table of taps behind the rings"""
    dp, cpl, carve = rm.fast_map(esz, D)
    return (carve + ring_bytes(T, D, esz)) * (rm.THREADS // dp) + 4 * T * D


def fast_takes(esz, D, chunk_len, T, general=False, no_fast=False, out_lo=0, out_esz=4):
    """does decode_fast.h serve the call: rolling rows' shapes, with rings and taps inside the budget"""
    lowdim = not general and D <= (4 if esz == 1 else 2)
    dp, cpl, carve = rm.fast_map(esz, D)
    return (not lowdim and not no_fast and cpl == 1 and 2 * D > dp and chunk_len * esz * 2 >= carve and (D * esz) % 16 == 0 and
            (chunk_len * esz) % 16 == 0 and out_lo % 16 == 0 and chunk_len * out_esz * 4096 < 0xf0000000 and fast_lds(esz, D, T) <= rm.FAST_LDS_BUDGET)


def fast_max_taps(esz, D):
    """the most taps (0: none) at which decode_fast.h's LDS fits the budget, by search over the formula above"""
    best = 0
    for T in range(1, MAX_TAPS + 1):
        if fast_lds(esz, D, T) <= rm.FAST_LDS_BUDGET:
            best = T
    return best
