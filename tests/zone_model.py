"""numpy model of zone-map pruning (sprintz_mi355x_zone_map / _zone_prune_box / _zone_prune_linear / _zone_expand, include/sprintz_mi355x.h),
applied to the ORIGINAL input -- decode is lossless and pinned elsewhere -- and written from the header's words, one chunk at a time in Python
integers where that is the plainest form.

A chunk's zone is its per-column unsigned minimum and maximum over EVERY element of the chunk (a partial last row counts) and its element
count zlen.  A chunk's class under a predicate is NONE (0: no row matches), ALL (1: every existing row matches) or DECODE (2: the decoder
must look); the survivors are the DECODE chunks in batch order."""
import numpy as np

import filter_model as fm

NONE, ALL, DECODE = 0, 1, 2
SPAN_LIMIT = 0xF0000000
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def zone_map(x, chunk_len, D, esz):
    """x: the flat original array -> (zmin [nchunks, D], zmax [nchunks, D], zlen int64 [nchunks]); a column without elements holds the
    identities (min all ones, max 0)"""
    x = np.asarray(x).ravel()
    top = (1 << (8 * esz)) - 1
    lens = fm.chunk_counts(x.size, chunk_len)
    zmin = np.full((len(lens), D), top, x.dtype)
    zmax = np.zeros((len(lens), D), x.dtype)
    for c, ne in enumerate(lens):
        v = x[c * chunk_len:c * chunk_len + ne]
        for d in range(min(D, ne)):
            zmin[c, d], zmax[c, d] = v[d::D].min(), v[d::D].max()
    return zmin, zmax, np.array(lens, np.int64)


def too_wide(first_offset, end_offset):
    return end_offset - first_offset >= SPAN_LIMIT


def by_len(zlen, D, wide):
    """what the element count and the span decide, or None"""
    if zlen < 0 or wide:
        return DECODE
    if zlen // D == 0:
        return NONE
    return None


def classify_box_chunk(zmin, zmax, zlen, lo, hi, mode, D, wide=False):
    k = by_len(int(zlen), D, wide)
    if k is not None:
        return k
    disjoint = [int(lo[d]) > int(hi[d]) or int(zmax[d]) < int(lo[d]) or int(zmin[d]) > int(hi[d]) for d in range(D)]
    inside = [int(lo[d]) <= int(zmin[d]) and int(zmax[d]) <= int(hi[d]) for d in range(D)]
    if mode == fm.ALL:
        return NONE if any(disjoint) else ALL if all(inside) else DECODE
    return ALL if any(inside) else NONE if all(disjoint) else DECODE


def classify_linear_chunk(zmin, zmax, zlen, w, bias, lo, hi, D, wide=False):
    k = by_len(int(zlen), D, wide)
    if k is not None:
        return k
    smin = int(bias) + sum(int(w[d]) * (int(zmin[d]) if int(w[d]) >= 0 else int(zmax[d])) for d in range(D))
    smax = int(bias) + sum(int(w[d]) * (int(zmax[d]) if int(w[d]) >= 0 else int(zmin[d])) for d in range(D))
    if smin < INT32_MIN or smax > INT32_MAX:
        return DECODE
    if lo > hi or smax < lo or smin > hi:
        return NONE
    return ALL if lo <= smin and smax <= hi else DECODE


def classify_box(zmin, zmax, zlen, lo, hi, mode, D, span=0):
    """-> uint8 [nchunks]"""
    wide = too_wide(0, span)
    return np.array([classify_box_chunk(zmin[c], zmax[c], zlen[c], lo, hi, mode, D, wide) for c in range(len(zlen))], np.uint8)


def classify_linear(zmin, zmax, zlen, w, bias, lo, hi, D, span=0):
    lo = INT32_MIN if lo is None else int(lo)
    hi = INT32_MAX if hi is None else int(hi)
    wide = too_wide(0, span)
    return np.array([classify_linear_chunk(zmin[c], zmax[c], zlen[c], w, bias, lo, hi, D, wide) for c in range(len(zlen))], np.uint8)


def positions(cls):
    """-> (pos int64 [nchunks + 1]: DECODE chunks in front of chunk c, pos[nchunks] = the survivors)"""
    return np.concatenate([[0], np.cumsum(np.asarray(cls) == DECODE)]).astype(np.int64)


def surviving_offsets(cls, offsets):
    """offsets int64 [nchunks + 1] -> [nchunks + 1]: the survivors' offsets in batch order, then the container's end"""
    offsets = np.asarray(offsets)
    keep = offsets[:-1][np.asarray(cls) == DECODE]
    return np.concatenate([keep, np.full(offsets.size - keep.size, offsets[-1])]).astype(offsets.dtype)


def all_mask(rows, MB):
    """the mask bytes of a chunk whose `rows` existing rows all match: bits r < rows set, the padding bits 0"""
    bits = np.zeros(MB * 8, np.uint8)
    bits[:rows] = 1
    return np.packbits(bits, bitorder="little")


def expand(cls, zlen, cmask, ccounts, crets, chunk_len, D):
    """the compact results of a filter on the survivors -> (mask uint8 [nchunks, MB], counts int64 [nchunks], rets int64 [nchunks])"""
    R, MB = fm.geometry(chunk_len, D)
    n = len(cls)
    mask, counts, rets = np.zeros((n, MB), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    s = 0
    for c in range(n):
        if cls[c] == DECODE:
            mask[c], counts[c], rets[c] = cmask[s], ccounts[s], crets[s] if zlen[c] >= 0 else zlen[c]      # damaged in the map: the map's code
            s += 1
            continue
        rets[c] = zlen[c]
        if cls[c] == ALL:
            counts[c] = int(zlen[c]) // D
            mask[c] = all_mask(int(counts[c]), MB)
    return mask, counts, rets
