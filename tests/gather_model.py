"""numpy model of gather rows (sprintz_mi355x_gather_rows, include/sprintz_mi355x.h): which pieces -- (chunk, rows of it,
place in the range) -- a range of batch rows falls into, which ranges cannot be delivered, and the expected samples, which
are slices of the ORIGINAL input (decode is lossless and pinned elsewhere)."""
import numpy as np

E_INVALID = -1          # SPRINTZ_E_INVALID: the range needs a row that does not exist


def max_pieces(rows, R):
    """P: the most chunks a range of `rows` rows can touch, chunks holding R rows"""
    return (rows + R - 2) // R + 1


def pieces(starts, rows, R, nchunks, stream_rows):
    """starts: batch rows (row g is row g % R of chunk g // R); stream_rows[c]: the rows chunk c's stream holds (R, fewer in
    a short last chunk).  -> (per range the list of its pieces (chunk, lo, hi, out_row): rows [lo, hi) of `chunk` land at
    rows [out_row, out_row + hi - lo) of the range; per range the expected d_rets entry: `rows`, or E_INVALID if the range
    needs a chunk >= nchunks or a row its chunk's stream does not hold -- its pieces are then those that do exist)."""
    rows, R, nchunks = int(rows), int(R), int(nchunks)
    all_pieces, rets = [], []
    for g0 in (int(s) for s in starts):
        c0, first = divmod(g0, R)
        end = first + rows                      # the range, in rows from row 0 of chunk c0
        ps, ok = [], True
        k = 0
        while k * R < end:
            c = c0 + k
            lo = max(first, k * R) - k * R
            hi = min(end, (k + 1) * R) - k * R
            if c >= nchunks:
                ok = False
                break
            have = int(stream_rows[c])
            if hi > have:
                ok = False
                hi = have
            if lo < hi:
                ps.append((c, lo, hi, k * R + lo - first))
            k += 1
        all_pieces.append(ps)
        rets.append(rows if ok else E_INVALID)
    return all_pieces, np.array(rets, np.int64)


def stream_rows(n, chunk_len, ndims):
    """whole rows held by each chunk's stream of a batch of n elements"""
    nchunks = -(-n // chunk_len)
    return np.array([min(chunk_len, n - c * chunk_len) // ndims for c in range(nchunks)], np.int64)


def expected(x, starts, rows, ndims=None):
    """x: the original array, [total_rows, ndims] (or flat with ndims given; a partial last row is dropped).  -> ([N, rows,
    ndims] with the rows that exist, zeros elsewhere; bool [N]: the range lies inside the batch)"""
    x = np.ascontiguousarray(x)
    if x.ndim == 1:
        x = x[: x.size // ndims * ndims].reshape(-1, ndims)
    total = x.shape[0]
    starts = np.asarray(starts, dtype=np.uint64).astype(object)
    out = np.zeros((len(starts), rows, x.shape[1]), x.dtype)
    ok = np.zeros(len(starts), bool)
    for i, g0 in enumerate(starts):
        g0 = int(g0)
        if g0 + rows <= total:
            out[i] = x[g0:g0 + rows]
            ok[i] = True
        elif g0 < total:
            out[i, : total - g0] = x[g0:]
    return out, ok
