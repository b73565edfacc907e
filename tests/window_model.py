"""numpy model of the windowed query (sprintz_mi355x_query_windows, include/sprintz_mi355x.h): chunk-relative windows
with their identities, windows over the batch's rows, and the fold of one-window-a-chunk results into the latter
(ChunkedCodec.query_windows).  The tests compare the device with this model applied to the ORIGINAL input: decode is
lossless, so the samples decompress_batch writes are the input's."""
import numpy as np


def _ident_min(esz):
    return (1 << (8 * esz)) - 1


def chunk_windows(x, chunk_len, ndims, window_rows):
    """x: the flat input (uint8 / uint16).  -> (min, max, sum) shaped [nchunks, nwin, ndims]; element e of chunk c sits in
    column e % ndims and window (e // ndims) // window_rows; empty windows hold min = all ones, max = 0, sum = 0."""
    x = np.ascontiguousarray(x).reshape(-1)
    esz = x.dtype.itemsize
    D, W = int(ndims), int(window_rows)
    n = x.size
    nchunks = -(-n // chunk_len)
    R = -(-chunk_len // D)
    nwin = -(-R // W)
    mn = np.full((nchunks, nwin, D), _ident_min(esz), x.dtype)
    mx = np.zeros((nchunks, nwin, D), x.dtype)
    sm = np.zeros((nchunks, nwin, D), np.uint64)
    i = np.arange(n, dtype=np.int64)
    c, e = i // chunk_len, i % chunk_len
    idx = (c, (e // D) // W, e % D)
    np.minimum.at(mn, idx, x)
    np.maximum.at(mx, idx, x)
    np.add.at(sm, idx, x.astype(np.uint64))
    return mn, mx, sm


def global_windows(x, ndims, window_rows):
    """windows over the batch's rows: window w covers rows [w W, min((w+1) W, rows)), rows = ceil(n / ndims).
    -> dict of [nwindows, ndims]: min / max (input dtype), sum / count (int64), mean (float64, nan where count is 0)"""
    x = np.ascontiguousarray(x).reshape(-1)
    D, W = int(ndims), int(window_rows)
    n = x.size
    rows = -(-n // D)
    nw = -(-rows // W)
    mn = np.full((nw, D), _ident_min(x.dtype.itemsize), x.dtype)
    mx = np.zeros((nw, D), x.dtype)
    sm = np.zeros((nw, D), np.int64)
    cnt = np.zeros((nw, D), np.int64)
    i = np.arange(n, dtype=np.int64)
    idx = ((i // D) // W, i % D)
    np.minimum.at(mn, idx, x)
    np.maximum.at(mx, idx, x)
    np.add.at(sm, idx, x.astype(np.int64))
    np.add.at(cnt, idx, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sm / cnt
    return {"min": mn, "max": mx, "sum": sm, "count": cnt, "mean": mean}


def kernel_window(chunk_len, ndims, window_rows):
    """the chunk window ChunkedCodec.query_windows asks the kernel for, and the chunks that fold into one global window
    (None where the shape has no global windows)"""
    D, W = int(ndims), int(window_rows)
    if chunk_len % D:
        return None
    R = chunk_len // D
    if R % W == 0:
        return W, 1
    if W % R == 0:
        return -(-R // 8) * 8, W // R
    return None


def fold(per_chunk, n, chunk_len, ndims, window_rows):
    """(min, max, sum) of chunk_windows at kernel_window's window -> the global windows' min / max / sum"""
    mn, mx, sm = per_chunk
    D, W = int(ndims), int(window_rows)
    kw, f = kernel_window(chunk_len, D, W)
    rows = -(-n // D)
    nw = -(-rows // W)
    nchunks = mn.shape[0]
    if f == 1:
        return {"min": mn.reshape(-1, D)[:nw], "max": mx.reshape(-1, D)[:nw], "sum": sm.reshape(-1, D)[:nw].astype(np.int64)}
    pad = nw * f - nchunks
    ident = _ident_min(mn.dtype.itemsize)
    pm = np.concatenate([mn.reshape(nchunks, D), np.full((pad, D), ident, mn.dtype)]).reshape(nw, f, D)
    px = np.concatenate([mx.reshape(nchunks, D), np.zeros((pad, D), mx.dtype)]).reshape(nw, f, D)
    ps = np.concatenate([sm.reshape(nchunks, D), np.zeros((pad, D), sm.dtype)]).reshape(nw, f, D)
    return {"min": pm.min(axis=1), "max": px.max(axis=1), "sum": ps.sum(axis=1).astype(np.int64)}


def brute_chunk_windows(x, chunk_len, ndims, window_rows):
    """the same as chunk_windows, one element at a time"""
    esz = np.asarray(x).dtype.itemsize
    x = list(np.asarray(x).reshape(-1))
    D, W = int(ndims), int(window_rows)
    nchunks = -(-len(x) // chunk_len)
    R = -(-chunk_len // D)
    nwin = -(-R // W)
    top = (1 << (8 * esz)) - 1
    mn = [[[top] * D for _ in range(nwin)] for _ in range(nchunks)]
    mx = [[[0] * D for _ in range(nwin)] for _ in range(nchunks)]
    sm = [[[0] * D for _ in range(nwin)] for _ in range(nchunks)]
    for c in range(nchunks):
        for e, v in enumerate(x[c * chunk_len:(c + 1) * chunk_len]):
            w, d = (e // D) // W, e % D
            v = int(v)
            mn[c][w][d] = min(mn[c][w][d], v)
            mx[c][w][d] = max(mx[c][w][d], v)
            sm[c][w][d] += v
    return np.array(mn), np.array(mx), np.array(sm)


def brute_global_windows(x, ndims, window_rows):
    """the same as global_windows (without mean), one window and column at a time"""
    top = _ident_min(np.asarray(x).dtype.itemsize)
    x = [int(v) for v in np.asarray(x).reshape(-1)]
    D, W = int(ndims), int(window_rows)
    rows = -(-len(x) // D)
    nw = -(-rows // W)
    out = {k: [[None] * D for _ in range(nw)] for k in ("min", "max", "sum", "count")}
    for w in range(nw):
        for d in range(D):
            vals = [x[r * D + d] for r in range(w * W, min((w + 1) * W, rows)) if r * D + d < len(x)]
            out["count"][w][d] = len(vals)
            out["sum"][w][d] = sum(vals)
            out["min"][w][d] = min(vals) if vals else top
            out["max"][w][d] = max(vals) if vals else 0
    return out
