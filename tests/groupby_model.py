"""numpy model of group-by rows (sprintz_mi355x_groupby_rows, include/sprintz_mi355x.h), applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere -- written from the definition with np.add.at, and a brute-force form, one row at a time.  Neither goes
through tests/histogram_model.py.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot, W = 8 * itemsize.  Row r of chunk c
EXISTS if all D of its elements lie inside the chunk's element count (a partial last row is not a row); it is SELECTED if it exists and
(there is no mask or) bit r & 7 of mask[c, r >> 3] is set.  A selected row whose key column holds x has b = ((x - key_lo) mod 2^W) >>
shift; if b < nbins the row belongs to bin b of table c // H (H = 0: table 0) -- count[t, b] takes 1 and sum[t, b, d] takes x_d for every
column d, the key column too -- and otherwise the whole row is dropped."""
import numpy as np


def default_shift(esz, nbins):
    """the shift that makes nbins bins cover the element range (one bin: the largest shift there is, W - 1)"""
    return min(max(8 * esz - max(nbins - 1, 0).bit_length(), 0), 8 * esz - 1)


def groupby_rows(x, chunk_len, D, key, mask=None, key_lo=0, shift=0, nbins=256, H=0):
    """x: the flat original array; mask: uint8 [nchunks, MB] or None.  -> (count uint64 [ntables, nbins], sum uint64 [ntables, nbins, D])"""
    assert chunk_len % D == 0 and 0 <= key < D
    x = np.asarray(x).ravel()
    W = 8 * x.dtype.itemsize
    assert 0 <= shift < W and 1 <= nbins <= 1 << (W - shift) and 0 <= key_lo < 1 << W
    nchunks = -(-x.size // chunk_len)
    ntables = -(-nchunks // H) if H else 1
    count = np.zeros((ntables, nbins), np.uint64)
    total = np.zeros((ntables, nbins, D), np.uint64)
    for c in range(nchunks):
        v = x[c * chunk_len:(c + 1) * chunk_len]
        rows = v[:v.size // D * D].reshape(-1, D).astype(np.uint64)          # the rows that exist
        keep = np.ones(rows.shape[0], bool)
        if mask is not None:
            keep = np.unpackbits(np.asarray(mask[c], np.uint8), bitorder="little")[:rows.shape[0]].astype(bool)
        b = ((rows[:, key].astype(np.int64) - int(key_lo)) % (1 << W)) >> shift
        keep &= b < nbins
        t = c // H if H else 0
        np.add.at(count[t], b[keep], np.uint64(1))
        np.add.at(total[t], b[keep], rows[keep])
    return count, total


def groupby_rows_brute(x, chunk_len, D, key, mask=None, key_lo=0, shift=0, nbins=256, H=0):
    """the same definition, one row at a time, in Python integers"""
    x = np.asarray(x).ravel()
    W = 8 * x.dtype.itemsize
    R = chunk_len // D
    nchunks = -(-x.size // chunk_len)
    ntables = -(-nchunks // H) if H else 1
    count = [[0] * nbins for _ in range(ntables)]
    total = [[[0] * D for _ in range(nbins)] for _ in range(ntables)]
    for c in range(nchunks):
        ne = min(chunk_len, x.size - c * chunk_len)
        for r in range(R):
            if (r + 1) * D > ne:
                break
            if mask is not None and not (int(mask[c][r >> 3]) >> (r & 7)) & 1:
                continue
            row = [int(e) for e in x[c * chunk_len + r * D:c * chunk_len + (r + 1) * D]]
            b = ((row[key] - key_lo) % (1 << W)) >> shift
            if b >= nbins:
                continue
            t = c // H if H else 0
            count[t][b] += 1
            for d in range(D):
                total[t][b][d] += row[d]
    return np.array(count, np.uint64).reshape(ntables, nbins), np.array(total, np.uint64).reshape(ntables, nbins, D)


def mean(count, total):
    """float64 sum / count, NaN where count is 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count[..., None] > 0, total.astype(np.float64) / count[..., None].astype(np.float64), np.nan)
