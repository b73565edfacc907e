"""numpy model of aggregate rows (sprintz_mi355x_aggregate_rows, include/sprintz_mi355x.h), applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere -- and a one-row-at-a-time brute force of the same definition.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot, W rows a window, nwin = ceil(R / W)
windows a chunk slot.  Row r of chunk c EXISTS if all D of its elements lie inside the chunk's element count (a partial last row is not
a row); it is SELECTED if it exists and bit r & 7 of mask[c, r >> 3] is set.  Window w of chunk c takes the selected rows r with
r // W == w: per column their unsigned min / max / sum, and their number.  A window with no selected row holds the identities: min all
ones, max 0, sum 0, count 0."""
import numpy as np

import filter_model as fm


def ident_min(esz):
    return (1 << (8 * esz)) - 1


def selected(mask, n, chunk_len, D):
    """-> bool [nchunks, R]: the rows that exist and whose bits are set"""
    R = chunk_len // D
    bits = np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R].astype(bool)
    for c, ne in enumerate(fm.chunk_counts(n, chunk_len)):
        bits[c, ne // D:] = False
    return bits


def aggregate_rows(x, chunk_len, D, mask, W):
    """x: the flat original array; mask: uint8 [nchunks, MB].  -> dict: min / max (x's dtype) and sum (uint64) [nchunks, nwin, D],
    count (uint32) [nchunks, nwin]"""
    assert chunk_len % D == 0 and W % 8 == 0 and W >= 8
    x = np.asarray(x).ravel()
    R = chunk_len // D
    nwin = -(-R // W)
    sel = selected(mask, x.size, chunk_len, D)
    nchunks = sel.shape[0]
    top = ident_min(x.dtype.itemsize)
    # every chunk slot padded to nwin * W rows; a row that is not selected holds the identity of the reduction it enters
    v = np.zeros((nchunks, nwin * W, D), x.dtype)
    s = np.zeros((nchunks, nwin * W), bool)
    s[:, :R] = sel
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        v[c, :ne // D] = x[c * chunk_len:c * chunk_len + ne // D * D].reshape(-1, D)
    v = v.reshape(nchunks, nwin, W, D)
    s = s.reshape(nchunks, nwin, W, 1)
    return {"min": np.where(s, v, x.dtype.type(top)).min(axis=2), "max": np.where(s, v, x.dtype.type(0)).max(axis=2),
            "sum": np.where(s, v, x.dtype.type(0)).astype(np.uint64).sum(axis=2), "count": s.sum(axis=(2, 3)).astype(np.uint32)}


def aggregate_rows_brute(x, chunk_len, D, mask, W):
    """the same definition, one row at a time"""
    x = np.asarray(x).ravel()
    esz = x.dtype.itemsize
    R = chunk_len // D
    nwin = -(-R // W)
    lens = fm.chunk_counts(x.size, chunk_len)
    top = ident_min(esz)
    mn = [[[top] * D for _ in range(nwin)] for _ in lens]
    mx = [[[0] * D for _ in range(nwin)] for _ in lens]
    sm = [[[0] * D for _ in range(nwin)] for _ in lens]
    cnt = [[0] * nwin for _ in lens]
    for c, ne in enumerate(lens):
        for r in range(R):
            if (r + 1) * D > ne or not (int(mask[c][r >> 3]) >> (r & 7)) & 1:
                continue
            w = r // W
            cnt[c][w] += 1
            for d in range(D):
                v = int(x[c * chunk_len + r * D + d])
                mn[c][w][d] = min(mn[c][w][d], v)
                mx[c][w][d] = max(mx[c][w][d], v)
                sm[c][w][d] += v
    return {"min": np.array(mn, x.dtype).reshape(len(lens), nwin, D), "max": np.array(mx, x.dtype).reshape(len(lens), nwin, D),
            "sum": np.array(sm, np.uint64).reshape(len(lens), nwin, D), "count": np.array(cnt, np.uint32).reshape(len(lens), nwin)}


def global_windows(x, chunk_len, D, mask, W):
    """windows over the batch's rows (chunk c holds batch rows [c R, (c + 1) R)): window w covers rows [w W, (w + 1) W), w <
    ceil(ceil(n / D) / W).  -> dict of min / max (x's dtype), sum / count (int64) [nwindows, D] / [nwindows], mean (float64, nan
    where count is 0)"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    sel = selected(mask, x.size, chunk_len, D)
    rows = -(-x.size // D)
    nw = -(-rows // W)
    mn = np.full((nw, D), ident_min(x.dtype.itemsize), x.dtype)
    mx = np.zeros((nw, D), x.dtype)
    sm = np.zeros((nw, D), np.int64)
    cnt = np.zeros(nw, np.int64)
    for c in range(sel.shape[0]):
        r = np.flatnonzero(sel[c])
        if r.size == 0:
            continue
        v = x[c * chunk_len:(c + 1) * chunk_len]
        v = v[:v.size // D * D].reshape(-1, D)[r]
        w = (c * R + r) // W
        np.minimum.at(mn, w, v)
        np.maximum.at(mx, w, v)
        np.add.at(sm, w, v.astype(np.int64))
        np.add.at(cnt, w, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sm / cnt[:, None]
    return {"min": mn, "max": mx, "sum": sm, "count": cnt, "mean": mean}
