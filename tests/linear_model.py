"""numpy model of linear filter rows (sprintz_mi355x_filter_linear, include/sprintz_mi355x.h), applied to the ORIGINAL input -- decode
is lossless and pinned elsewhere -- computed in int64 on the whole batch, and a one-row-at-a-time brute force of the same definition.

chunk_len % D == 0; chunk c holds batch rows [c R, (c + 1) R), R = chunk_len / D; a partial last row of the batch is not a row.  For
batch row g, with x the unsigned element:

    s(g) = bias + sum_d w[d] x[g, d] + sum_d u[d] x[p(g), d],   p(g) = g - 1 for g > 0, p(0) = 0
    row g matches  <=>  lo <= s(g) <= hi        (signed, inclusive; lo > hi matches nothing)

The kernel's s wraps modulo 2^32; the model wraps the same way (wrap32), so the two agree for every int32 weight -- and s is the plain
integer wherever B = |bias| + (2^W - 1) sum_d (|w[d]| + |u[d]|) < 2^31 (bound_B).  u = None: no lag term.  The output is filter rows'."""
import numpy as np

import filter_model as fm

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def wrap32(s):
    """int64 -> the value its low 32 bits have as two's complement"""
    return ((np.asarray(s, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def bound_B(esz, w, u=None, bias=0):
    return abs(int(bias)) + ((1 << (8 * esz)) - 1) * (sum(abs(int(e)) for e in w) + sum(abs(int(e)) for e in (u if u is not None else ())))


def sums(x, D, w, u=None, bias=0, self_rows=()):
    """s(g) of every whole row of the flat batch x, wrapped to int32 range, int64 [rows].  self_rows: rows that take THEMSELVES as
    predecessor instead of the row in front (row 0 always does) -- what the decode launch computes for a chunk's first row before the
    seam pass."""
    x = np.asarray(x).astype(np.int64).ravel()
    rows = x.size // D
    v = x[:rows * D].reshape(rows, D)
    s = np.full(rows, int(bias), np.int64) + v @ np.asarray(w, np.int64).reshape(D)
    if u is not None and rows:
        p = np.concatenate([v[:1], v[:-1]])
        for g in self_rows:
            if g < rows:
                p[g] = v[g]
        s = s + p @ np.asarray(u, np.int64).reshape(D)
    return wrap32(s)


def pack(match, n, chunk_len, D):
    """a bool per whole batch row -> (mask uint8 [nchunks, MB], counts int64 [nchunks]) in filter rows' layout"""
    assert chunk_len % D == 0
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    bits = np.zeros((nchunks, MB * 8), np.uint8)
    for c in range(nchunks):
        m = match[c * R:(c + 1) * R]
        bits[c, :m.size] = m
    return np.packbits(bits, axis=1, bitorder="little"), bits.sum(axis=1).astype(np.int64)


def filter_linear(x, chunk_len, D, w, lo=None, hi=None, u=None, bias=0, self_rows=()):
    """-> (mask uint8 [nchunks, MB], counts int64 [nchunks])"""
    lo = INT32_MIN if lo is None else int(lo)
    hi = INT32_MAX if hi is None else int(hi)
    s = sums(x, D, w, u, bias, self_rows)
    return pack((s >= lo) & (s <= hi), np.asarray(x).size, chunk_len, D)


def filter_change(x, chunk_len, D, col, lo=None, hi=None, self_rows=()):
    e = np.zeros(D, np.int64)
    e[col] = 1
    return filter_linear(x, chunk_len, D, e, lo, hi, -e, 0, self_rows)


def filter_linear_brute(x, chunk_len, D, w, lo=None, hi=None, u=None, bias=0):
    """the same definition, one row at a time, in Python integers"""
    x = [int(e) for e in np.asarray(x).ravel()]
    lo = INT32_MIN if lo is None else int(lo)
    hi = INT32_MAX if hi is None else int(hi)
    assert chunk_len % D == 0
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-len(x) // chunk_len)
    mask = np.zeros((nchunks, MB), np.uint8)
    counts = np.zeros(nchunks, np.int64)
    for g in range(len(x) // D):
        p = g - 1 if g > 0 else 0
        s = int(bias)
        for d in range(D):
            s += int(w[d]) * x[g * D + d]
            if u is not None:
                s += int(u[d]) * x[p * D + d]
        s = (s + (1 << 31)) % (1 << 32) - (1 << 31)
        if lo <= s <= hi:
            c, r = divmod(g, R)
            mask[c, r >> 3] |= 1 << (r & 7)
            counts[c] += 1
    return mask, counts
