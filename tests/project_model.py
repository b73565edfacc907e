"""The numpy model of project rows (sprintz_mi355x_project_rows, ChunkedCodec.project_rows): the only specification the mode has.

columns = (c_0 .. c_{K-1}) are K >= 1 distinct column numbers in 0 .. ndims - 1, in any order.  With R = chunk_len / ndims (chunk_len is a
multiple of ndims), batch row g is row g % R of chunk g // R -- the chunks lie back to back, so that is row g of the batch reshaped
[G, ndims], G = ceil(total_len / ndims) -- and

    out[g, j] = x[g, c_j]                                                  raw: the element type
              = float_model's value of x[g, c_j] with scale[j], offset[j]  a float format: float rows' rule, bit for bit

The output is dense, [G, K]: chunk c's rows start at output row c * R.  Where the batch ends mid-row, the elements of the last row that do
not exist hold 0 (the C entry does not write them: `written` says which places it writes).  Float results are returned as BITS, as
float_model returns them."""
import numpy as np

import float_model as fm

RAW = -1                                                   # the model's name for "the element type"; F32 / F16 / BF16 are float_model's


def check_columns(columns, ndims):
    cols = [int(c) for c in columns]
    assert cols and len(set(cols)) == len(cols) and all(0 <= c < ndims for c in cols), (columns, ndims)
    return cols


def slots(columns, ndims):
    """the slot table the library reads: int32 [ndims], slots[c_j] = j, -1 elsewhere"""
    s = np.full(ndims, -1, np.int32)
    for j, c in enumerate(check_columns(columns, ndims)):
        s[c] = j
    return s


def padded(x, ndims):
    """-> (the batch as [G, ndims] with zeros behind its last element, which elements exist [G, ndims])"""
    x = np.asarray(x).reshape(-1)
    G = -(-x.size // ndims)
    full = np.zeros(G * ndims, x.dtype)
    full[:x.size] = x
    return full.reshape(G, ndims), (np.arange(G * ndims) < x.size).reshape(G, ndims)


def written(n, ndims, columns):
    """bool [G, K]: the places of the output that the C entry writes -- those whose element exists"""
    cols = check_columns(columns, ndims)
    G = -(-n // ndims)
    return (np.arange(G * ndims) < n).reshape(G, ndims)[:, cols]


def project(x, chunk_len, ndims, columns, fmt=RAW, scale=None, offset=None, signed=False):
    """-> [G, K]: the element type for RAW, else the bits of the float format; 0 where the element does not exist"""
    assert chunk_len % ndims == 0
    cols = check_columns(columns, ndims)
    rows, exists = padded(x, ndims)
    sel = rows[:, cols]
    if fmt == RAW:
        assert scale is None and offset is None and not signed
        return sel.copy()
    K = len(cols)
    scale = np.ones(K, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(K)
    offset = np.zeros(K, np.float32) if offset is None else np.asarray(offset, np.float32).reshape(K)
    bits = fm.convert(sel, scale[None, :], offset[None, :], signed, fmt)
    bits[~exists[:, cols]] = 0
    return bits


def project_chunks(x, chunk_len, ndims, columns, fmt=RAW, scale=None, offset=None, signed=False):
    """the same, chunk by chunk and element by element: element e of chunk c is in row c * R + e // ndims and column e % ndims, and leaves
    at slot slots[e % ndims] of that output row"""
    x = np.asarray(x).reshape(-1)
    cols = check_columns(columns, ndims)
    K, R = len(cols), chunk_len // ndims
    s = slots(cols, ndims)
    G = -(-x.size // ndims)
    out = np.zeros((G, K), x.dtype if fmt == RAW else fm.BITS_DTYPE[fmt])
    scale = np.ones(K, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(K)
    offset = np.zeros(K, np.float32) if offset is None else np.asarray(offset, np.float32).reshape(K)
    for c in range(-(-x.size // chunk_len)):
        for e in range(min(chunk_len, x.size - c * chunk_len)):
            j = s[e % ndims]
            if j < 0:
                continue
            v = x[c * chunk_len + e]
            out[c * R + e // ndims, j] = v if fmt == RAW else fm.convert(np.array([v], x.dtype), scale[j], offset[j], signed, fmt)[0]
    return out


def fast_takes(esz, D, chunk_len, K, out_esz, general=False, no_fast=0, out_lo=0):
    """plan.h's rule for the mode, restated: does decode_fast.h serve the shape?  One column a lane (up to 64 columns, the power-of-two group
    more than half full), the plain decode's terms for the shape, and a projected block of whole 16-byte pieces within the descriptor's reach"""
    lowdim = (not general) and D <= (4 if esz == 1 else 2)
    dp = 4
    while dp < D and dp < 64:
        dp <<= 1
    if lowdim or no_fast or D > 64 or 2 * D <= dp:
        return False
    W = 8 * esz
    hb = 3 if W == 8 else 4
    unit = dp * 16
    blkmax = 8 * dp * esz
    cg = (2 * dp * hb + 7) // 8 + 2 * blkmax + 4
    ring = ((2 * (cg + 24) + 3 + unit - 1) // unit + 1) * unit + ((cg + 24 + 8 + 15) & ~15) + ((8 * D * esz + 15) & ~15) + 16
    return (chunk_len * esz * 2 >= ring and (8 * D * esz) % 16 == 0 and (chunk_len * esz) % 16 == 0 and out_lo % 16 == 0 and
            (8 * K * esz) % 16 == 0 and (chunk_len // D) * K * out_esz * 4096 < 0xf0000000)
