"""numpy model of filter rows (sprintz_mi355x_filter_rows / sprintz_mi355x_filter_row_ids, include/sprintz_mi355x.h), applied to the
ORIGINAL input -- decode is lossless and pinned elsewhere -- and a one-element-at-a-time brute force of the same definition.

Element e of chunk c is in row e // D and column e % D; a row EXISTS if all D of its elements lie inside the chunk's element count (a
partial last row is not a row).  A row matches under ALL if every column d has lo[d] <= x <= hi[d], under ANY if some column has
(unsigned, inclusive: lo[d] > hi[d] never matches).  Bit r & 7 of mask[c, r >> 3] is 1 iff row r of chunk c exists and matches."""
import numpy as np

ALL, ANY = 0, 1


def geometry(chunk_len, D):
    """-> (R rows a chunk slot, MB mask bytes a chunk slot)"""
    R = -(-chunk_len // D)
    return R, -(-R // 8)


def chunk_counts(n, chunk_len):
    """elements held by each chunk's stream of a batch of n elements"""
    nchunks = -(-n // chunk_len)
    return [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]


def filter_rows(x, chunk_len, D, lo, hi, mode):
    """x: the flat original array.  -> (mask uint8 [nchunks, MB], counts int64 [nchunks])"""
    x = np.asarray(x).astype(np.int64).ravel()
    lo = np.asarray(lo, np.int64).reshape(D)
    hi = np.asarray(hi, np.int64).reshape(D)
    R, MB = geometry(chunk_len, D)
    lens = chunk_counts(x.size, chunk_len)
    mask = np.zeros((len(lens), MB), np.uint8)
    counts = np.zeros(len(lens), np.int64)
    for c, ne in enumerate(lens):
        rows = ne // D
        v = x[c * chunk_len:c * chunk_len + rows * D].reshape(rows, D)
        ok = (v >= lo) & (v <= hi)
        m = ok.all(axis=1) if mode == ALL else ok.any(axis=1)
        bits = np.zeros(MB * 8, np.uint8)
        bits[:rows] = m
        mask[c] = np.packbits(bits, bitorder="little")
        counts[c] = int(m.sum())
    return mask, counts


def filter_rows_brute(x, chunk_len, D, lo, hi, mode):
    """the same definition, one element at a time"""
    x = [int(e) for e in np.asarray(x).ravel()]
    R, MB = geometry(chunk_len, D)
    lens = chunk_counts(len(x), chunk_len)
    mask = np.zeros((len(lens), MB), np.uint8)
    counts = np.zeros(len(lens), np.int64)
    for c, ne in enumerate(lens):
        for r in range(R):
            if (r + 1) * D > ne:                       # the row does not exist
                continue
            hits = 0
            for d in range(D):
                e = x[c * chunk_len + r * D + d]
                if int(lo[d]) <= e <= int(hi[d]):
                    hits += 1
            if hits == D if mode == ALL else hits > 0:
                mask[c, r >> 3] |= 1 << (r & 7)
                counts[c] += 1
    return mask, counts


def row_ids(mask, chunk_len, D, capacity=None, sentinel=-1):
    """filter_row_ids with the exclusive prefix sum of the chunks' counts as bases: the matching batch rows, ascending (chunk_len % D
    == 0; row g is row g % R of chunk g // R).  capacity: the ids array has that many entries, those past the total keep `sentinel`"""
    assert chunk_len % D == 0
    R = chunk_len // D
    bits = np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R]
    ids = np.flatnonzero(bits.reshape(-1)).astype(np.int64)     # row r of chunk c is entry c * R + r
    if capacity is None:
        return ids
    out = np.full(capacity, sentinel, np.int64)
    k = min(capacity, ids.size)
    out[:k] = ids[:k]
    return out


def neutral(esz, mode):
    """the bounds that leave a column out of the verdict: always under ALL, never under ANY -> (lo, hi)"""
    top = (1 << (8 * esz)) - 1
    return (0, top) if mode == ALL else (top, 0)
