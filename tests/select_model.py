"""numpy model of select rows (sprintz_mi355x_select_rows, include/sprintz_mi355x.h), applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere -- and a one-row-at-a-time brute force of the same definition.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot.  Row r of chunk c EXISTS if all D
of its elements lie inside the chunk's element count.  The i-th set bit of chunk c's mask, in ascending row order over the rows that
exist, is row r: its D elements land in output row bases[c] + i and c * R + r in the same entry of the ids; a place >= capacity is
dropped.  Nothing else is written: everything else keeps the sentinel."""
import numpy as np

import filter_model as fm


def counts(mask, n, chunk_len, D):
    """set bits of every chunk over the rows that exist -> int64 [nchunks]"""
    R = chunk_len // D
    bits = np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R]
    return np.array([int(bits[c, :ne // D].sum()) for c, ne in enumerate(fm.chunk_counts(n, chunk_len))], np.int64)


def prefix_bases(cnt):
    """the usual bases: the exclusive prefix sum of the counts"""
    cnt = np.asarray(cnt, np.int64)
    return np.cumsum(cnt) - cnt


def select_rows(x, chunk_len, D, mask, bases, capacity, out_rows=None, sentinel=0, id_sentinel=-1):
    """x: the flat original array; mask: uint8 [nchunks, MB]; bases: [nchunks]; out_rows: rows of the output arrays (default: capacity).
    -> (rows [out_rows, D] of x's dtype, ids int64 [out_rows]), `sentinel` / `id_sentinel` wherever nothing is written"""
    assert chunk_len % D == 0
    x = np.asarray(x).ravel()
    R = chunk_len // D
    out_rows = capacity if out_rows is None else out_rows
    rows = np.full((out_rows, D), sentinel, x.dtype)
    ids = np.full(out_rows, id_sentinel, np.int64)
    bits = np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R]
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        have = ne // D
        r = np.flatnonzero(bits[c, :have])
        place = int(bases[c]) + np.arange(r.size)
        keep = place < min(capacity, out_rows)
        v = x[c * chunk_len:c * chunk_len + have * D].reshape(have, D)
        rows[place[keep]] = v[r[keep]]
        ids[place[keep]] = c * R + r[keep]
    return rows, ids


def select_rows_brute(x, chunk_len, D, mask, bases, capacity, out_rows=None, sentinel=0, id_sentinel=-1):
    """the same definition, one row at a time"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    out_rows = capacity if out_rows is None else out_rows
    rows = np.full((out_rows, D), sentinel, x.dtype)
    ids = np.full(out_rows, id_sentinel, np.int64)
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        i = 0
        for r in range(R):
            if (r + 1) * D > ne or not (int(mask[c][r >> 3]) >> (r & 7)) & 1:
                continue
            p = int(bases[c]) + i
            i += 1
            if p < capacity and p < out_rows:
                for d in range(D):
                    rows[p, d] = x[c * chunk_len + r * D + d]
                ids[p] = c * R + r
    return rows, ids
