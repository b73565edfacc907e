"""numpy model of derive rows (sprintz_mi355x_derive_rows, ChunkedCodec.derive_rows): the only specification the mode has.  Applied to the
ORIGINAL input -- decode is lossless and pinned elsewhere.

chunk_len % D == 0; chunk c holds batch rows [c R, (c + 1) R), R = chunk_len / D; a partial last row of the batch is not a row.  For K forms
and batch row g, with x the unsigned element:

    s[g, k] = bias[k] + sum_d w[k, d] x[g, d] + sum_d u[k, d] x[p(g), d]      modulo 2^32, read as int32
    p(g) = g - 1; row 0's predecessor is itself, or the `prev` row where one is given

built on linear_model.sums, a form at a time (its self_rows are what the decode launch computes for a chunk's first row before the seam
pass).  u = None: no lag term, and prev is ignored.  The float formats convert s as float rows convert an element:

    z = fl32(fl32(float32(s) * scale[k]) + offset[k])       float32(s): int32 -> float32, round to nearest even; never one fma

and float_model.to_bits rounds z to the format.  Floats are returned as BITS: the tests compare bits, not values."""
import numpy as np

import float_model as flm
import linear_model as lm

I32 = -1                                    # the int32 format, next to float_model's F32 / F16 / BF16
FORMATS = (I32,) + flm.FORMATS
C_FORMAT = {I32: 0, flm.F32: 1, flm.F16: 2, flm.BF16: 3}          # SPRINTZ_DERIVE_*
OUT_BYTES = {I32: 4, **flm.OUT_BYTES}
BITS_DTYPE = {I32: np.uint32, **flm.BITS_DTYPE}


def sums(x, D, w, u=None, bias=None, prev=None, self_rows=()):
    """s[g, k] of every whole row of the flat batch x -> int64 [rows, K], each value in int32's range.  w, u: [K, D]; bias: [K] or None;
    prev: [D] (the row in front of row 0) or None; self_rows: rows that take themselves as predecessor (linear_model.sums)"""
    x = np.asarray(x).ravel()
    w = np.asarray(w, np.int64).reshape(-1, D)
    K = w.shape[0]
    u = None if u is None else np.asarray(u, np.int64).reshape(K, D)
    bias = np.zeros(K, np.int64) if bias is None else np.asarray(bias, np.int64).reshape(K)
    rows = x.size // D
    out = np.zeros((rows, K), np.int64)
    for k in range(K):
        s = lm.sums(x, D, w[k], None if u is None else u[k], int(bias[k]), self_rows)
        if u is not None and prev is not None and rows and 0 not in self_rows:
            # row 0 took itself: take that term out and put prev's in
            x0 = x[:D].astype(np.int64)
            s[0] = lm.wrap32(s[0] - x0 @ u[k] + np.asarray(prev).astype(np.int64).reshape(D) @ u[k])
        out[:, k] = s
    return out


def sums_brute(x, D, w, u=None, bias=None, prev=None):
    """the same definition, one row and one form at a time, in Python integers"""
    x = [int(e) for e in np.asarray(x).ravel()]
    K = len(w)
    rows = len(x) // D
    out = np.zeros((rows, K), np.int64)
    for g in range(rows):
        if g > 0:
            p = x[(g - 1) * D:g * D]
        elif prev is not None:
            p = [int(e) for e in np.asarray(prev).ravel()]
        else:
            p = x[:D]
        for k in range(K):
            s = 0 if bias is None else int(bias[k])
            for d in range(D):
                s += int(w[k][d]) * x[g * D + d]
                if u is not None:
                    s += int(u[k][d]) * p[d]
            out[g, k] = (s + (1 << 31)) % (1 << 32) - (1 << 31)
    return out


def convert(s, fmt, scale=None, offset=None):
    """s int64 [rows, K] in int32's range -> the output's BITS [rows, K]: uint32 for int32 and float32, uint16 for the 16-bit formats"""
    s = np.asarray(s, np.int64)
    if fmt == I32:
        return s.astype(np.int32).view(np.uint32)
    K = s.shape[1]
    scale = np.ones(K, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(K)
    offset = np.zeros(K, np.float32) if offset is None else np.asarray(offset, np.float32).reshape(K)
    f = s.astype(np.int32).astype(np.float32)           # int32 -> float32: round to nearest even
    return flm.to_bits(flm.affine(f, scale[None, :], offset[None, :]), fmt).reshape(s.shape)


def derive_rows(x, D, w, u=None, bias=None, fmt=I32, scale=None, offset=None, prev=None, self_rows=()):
    return convert(sums(x, D, w, u, bias, prev, self_rows), fmt, scale, offset)


def fast_ring(esz, D):
    """geom.h: decode_fast_lds_bytes on the one-column-a-lane mapping of D columns -> (lanes a chunk, the plain decode's bytes of LDS a group)"""
    dp = 4
    while dp < D and dp < 64:
        dp <<= 1
    hb = 3 if esz == 1 else 4
    unit = dp * 16
    blkmax = 8 * dp * esz
    cg = (2 * dp * hb + 7) // 8 + 2 * blkmax + 4
    return dp, ((2 * (cg + 24) + 3 + unit - 1) // unit + 1) * unit + ((cg + 24 + 8 + 15) & ~15) + ((8 * D * esz + 15) & ~15) + 16


def fast_stride(esz, D, K, out_esz):
    """the group's LDS in this mode: the plain decode's, with the staging grown to the derived block (8 K out_esz bytes) where that is larger"""
    dp, ring = fast_ring(esz, D)
    return ring + max(0, 8 * K * out_esz - ((8 * D * esz + 15) & ~15))


def fast_takes(esz, D, chunk_len, K, out_esz, general=False, no_fast=0, out_lo=0):
    """plan.h's rule for the mode, restated: does decode_fast.h serve the shape?  One column a lane (up to 64 columns, the power-of-two group
    more than half full), the plain decode's terms for the shape, a 16-byte aligned output, the derived slots within the descriptor's reach,
    and the groups' carves with the table of weights within 80 KB of LDS"""
    lowdim = (not general) and D <= (4 if esz == 1 else 2)
    dp, ring = fast_ring(esz, D)
    if lowdim or no_fast or D > 64 or 2 * D <= dp:
        return False
    return (chunk_len * esz * 2 >= ring and (8 * D * esz) % 16 == 0 and (chunk_len * esz) % 16 == 0 and out_lo % 16 == 0 and
            (chunk_len // D) * K * out_esz * 4096 < 0xf0000000 and fast_stride(esz, D, K, out_esz) * (256 // dp) + K * D * 8 <= 80 * 1024)


def form_params(K):
    """form k takes pair k % 8 of float_model.PAIRS -> (scale, offset) float32 [K]"""
    return flm.column_params(K)
