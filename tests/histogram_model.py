"""numpy model of histogram rows (sprintz_mi355x_histogram_rows, include/sprintz_mi355x.h) and of ChunkedCodec.quantiles, applied to
the ORIGINAL input -- decode is lossless and pinned elsewhere -- written from the definitions, and brute-force forms of both.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot, W = 8 * itemsize.  Row r of chunk c
EXISTS if all D of its elements lie inside the chunk's element count (a partial last row is not a row); it is SELECTED if it exists and
(there is no mask or) bit r & 7 of mask[c, r >> 3] is set.  Value x of column d in a selected row has t = (x - lo[d]) mod 2^W and is
counted in bin t >> shift of histogram c // H (H = 0: histogram 0) if that is below nbins, and nowhere otherwise."""
import math

import numpy as np

import filter_model as fm


def selected(mask, n, chunk_len, D):
    """-> bool [nchunks, R]: the rows that exist and (mask is None or) whose bits are set"""
    R = chunk_len // D
    lens = fm.chunk_counts(n, chunk_len)
    if mask is None:
        bits = np.ones((len(lens), R), bool)
    else:
        bits = np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R].astype(bool)
    for c, ne in enumerate(lens):
        bits[c, ne // D:] = False
    return bits


def default_shift(esz, nbins):
    """the shift that makes nbins bins cover the element range (one bin: the largest shift there is, W - 1)"""
    return min(max(8 * esz - max(nbins - 1, 0).bit_length(), 0), 8 * esz - 1)


def histogram_rows(x, chunk_len, D, mask=None, lo=None, shift=0, nbins=256, H=0):
    """x: the flat original array; mask: uint8 [nchunks, MB] or None; lo: [D] or None.  -> uint64 [ngroups, D, nbins]"""
    assert chunk_len % D == 0
    x = np.asarray(x).ravel()
    W = 8 * x.dtype.itemsize
    assert 0 <= shift < W and 1 <= nbins <= 1 << (W - shift)
    sel = selected(mask, x.size, chunk_len, D)
    nchunks = sel.shape[0]
    ngroups = -(-nchunks // H) if H else 1
    lo = np.zeros(D, np.int64) if lo is None else np.asarray(lo, np.int64).reshape(D)
    hist = np.zeros((ngroups, D, nbins), np.uint64)
    for c in range(nchunks):
        r = np.flatnonzero(sel[c])
        if r.size == 0:
            continue
        v = x[c * chunk_len:(c + 1) * chunk_len]
        v = v[:v.size // D * D].reshape(-1, D)[r].astype(np.int64)
        b = ((v - lo[None, :]) % (1 << W)) >> shift
        g = c // H if H else 0
        for d in range(D):
            bd = b[:, d]
            hist[g, d] += np.bincount(bd[bd < nbins], minlength=nbins).astype(np.uint64)
    return hist


def histogram_rows_brute(x, chunk_len, D, mask=None, lo=None, shift=0, nbins=256, H=0):
    """the same definition, one sample at a time"""
    x = np.asarray(x).ravel()
    W = 8 * x.dtype.itemsize
    lens = fm.chunk_counts(x.size, chunk_len)
    R = chunk_len // D
    ngroups = -(-len(lens) // H) if H else 1
    hist = np.zeros((ngroups, D, nbins), np.uint64)
    for c, ne in enumerate(lens):
        for r in range(R):
            if (r + 1) * D > ne:
                continue
            if mask is not None and not (int(mask[c][r >> 3]) >> (r & 7)) & 1:
                continue
            for d in range(D):
                t = (int(x[c * chunk_len + r * D + d]) - (0 if lo is None else int(lo[d]))) % (1 << W)
                if (t >> shift) < nbins:
                    hist[c // H if H else 0, d, t >> shift] += np.uint64(1)
    return hist


def selected_values(x, chunk_len, D, mask=None):
    """-> [n, D]: the selected rows of the batch"""
    x = np.asarray(x).ravel()
    sel = selected(mask, x.size, chunk_len, D)
    rows = []
    for c in range(sel.shape[0]):
        v = x[c * chunk_len:(c + 1) * chunk_len]
        rows.append(v[:v.size // D * D].reshape(-1, D)[np.flatnonzero(sel[c])])
    return np.concatenate(rows) if rows else np.zeros((0, D), x.dtype)


def quantile_index(q, n):
    """the index of quantile q among n sorted values: max(ceil(q n), 1) - 1"""
    return max(int(math.ceil(float(q) * float(n))), 1) - 1


def quantiles(x, chunk_len, D, q, mask=None):
    """the sort definition: per column the sorted selected values at quantile_index(q, n).  -> x's dtype [len(q), D]; ValueError for n == 0"""
    v = selected_values(x, chunk_len, D, mask)
    n = v.shape[0]
    if n == 0:
        raise ValueError("no row is selected")
    s = np.sort(v, axis=0)
    return np.stack([s[quantile_index(qi, n)] for qi in q])


def quantiles_from_histogram(hist, q):
    """the same from a full-resolution histogram [D, 2^W] of the selected values: the first value whose cumulative count exceeds the index"""
    cum = np.cumsum(hist.astype(np.int64), axis=1)
    out = np.zeros((len(q), hist.shape[0]), np.int64)
    for d in range(hist.shape[0]):
        n = int(cum[d, -1])
        if n == 0:
            raise ValueError("no row is selected")
        for i, qi in enumerate(q):
            out[i, d] = np.searchsorted(cum[d], quantile_index(qi, n), side="right")
    return out
