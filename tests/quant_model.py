"""The numpy model of compress floats (sprintz_mi355x_compress_batch_float / _float_dense, ChunkedCodec.compress_floats): the quantisation the
encoders apply to a float source while they load it, restated from the header.

Element e of the source is in column d = e % ndims (chunk_len % ndims == 0; a short last chunk may end mid-row).  For the source element
x -- float32, float16 or bfloat16 --

    v = float32(x)                                     exact for the 16-bit formats
    t = fl32(fl32(v - offset[d]) * inv_scale[d])       two float32 operations, never contracted
    r = rint(t), ties to even -- or floor(t)
    q = 0 where r is NaN, else clamp(r, LO, HI)        LO / HI = 0 / 2^W - 1, or -2^(W-1) / 2^(W-1) - 1 where `signed`

and q is handed to the encoder as a W-bit two's-complement element: the model returns it as uint8 / uint16, the tensor whose compress() the
float call must equal byte for byte."""
import numpy as np

F32, F16, BF16 = 0, 1, 2
FORMATS = (F32, F16, BF16)
NAMES = {F32: "float32", F16: "float16", BF16: "bfloat16"}
SRC_BYTES = {F32: 4, F16: 2, BF16: 2}
DTYPES = {8: np.uint8, 16: np.uint16}

# (inv_scale, offset): identity; the 8-bit and the 16-bit range of [0, 1) -- the second with an offset of half a step; a typical
# quantisation; an inverse scale that overflows every product; a negative one with a tiny offset; one whose products are ties;
# a huge one that lifts the smallest float32 into range, with a subnormal offset
PAIRS = [(1.0, 0.0), (255.0, 0.0), (65535.0, -0.5 / 65535), (10.0, -3276.8), (3e38, 0.0), (-7.3, 1e-30), (0.5, 0.25), (2.0 ** 127, 2.0 ** -140)]


def column_params(ndims):
    """column d takes pair d % 8 of PAIRS, so that a value quantised with another column's parameters shows -> (inv_scale, offset) float32 [ndims]"""
    inv = np.array([PAIRS[d % len(PAIRS)][0] for d in range(ndims)], np.float32)
    off = np.array([PAIRS[d % len(PAIRS)][1] for d in range(ndims)], np.float32)
    return inv, off


def limits(W, signed):
    return (-(1 << (W - 1)), (1 << (W - 1)) - 1) if signed else (0, (1 << W) - 1)


def source_bits(x, fmt):
    """float values -> the source as the device sees it: float32, or the bits (uint16) of float16 / of bfloat16 rounded to nearest even"""
    x = np.asarray(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if fmt == F32:
            return np.ascontiguousarray(x, np.float32)
        if fmt == F16:
            return x.astype(np.float16).view(np.uint16)
        u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, np.uint16(0x7FC0), r).astype(np.uint16)


def source_values(src, fmt):
    """source_bits' result -> float32, exactly"""
    if fmt == F32:
        return np.asarray(src, np.float32)
    src = np.asarray(src, np.uint16)
    if fmt == F16:
        return src.view(np.float16).astype(np.float32)
    return (src.astype(np.uint32) << 16).view(np.float32)


def quantize(v, inv_scale, offset, W, signed=False, floor=False):
    """elementwise: v (float32) and inv_scale / offset broadcast against each other -> q as uint8 / uint16"""
    v = np.asarray(v, np.float32)
    lo, hi = limits(W, signed)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = (v - np.asarray(offset, np.float32)).astype(np.float32)
        t = (s * np.asarray(inv_scale, np.float32)).astype(np.float32)
        r = np.floor(t) if floor else np.rint(t)
        c = np.where(r < lo, np.float32(lo), np.where(r > hi, np.float32(hi), r))
        q = np.where(np.isnan(r), np.float32(0), c).astype(np.int64)
    return (q & ((1 << W) - 1)).astype(DTYPES[W])


def compress_floats(v, chunk_len, ndims, W, inv_scale=None, offset=None, signed=False, floor=False):
    """the batch v (float32 values of the source, its chunks back to back, the last one possibly short) -> q of v.size elements.  Element e
    of chunk c is element c * chunk_len + e of v and of the result, in column e % ndims"""
    assert chunk_len % ndims == 0
    v = np.asarray(v, np.float32).reshape(-1)
    inv = np.ones(ndims, np.float32) if inv_scale is None else np.asarray(inv_scale, np.float32).reshape(ndims)
    off = np.zeros(ndims, np.float32) if offset is None else np.asarray(offset, np.float32).reshape(ndims)
    d = (np.arange(v.size, dtype=np.int64) % chunk_len) % ndims
    return quantize(v, inv[d], off[d], W, signed, floor)


def quantize_one(v, inv, off, W, signed, floor):
    """the definition on one element, with Python's own arithmetic on float32 values: the brute force the array form is checked against"""
    import math
    lo, hi = limits(W, signed)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = float(np.float32(np.float32(np.float32(v) - np.float32(off)) * np.float32(inv)))
    if math.isnan(t):
        q = 0
    elif math.isinf(t):
        q = hi if t > 0 else lo
    else:
        if floor:
            r = math.floor(t)
        else:
            r = math.floor(t)
            frac = t - r                                   # exact: t is a float32
            if frac > 0.5 or (frac == 0.5 and r % 2 == 1):
                r += 1
        q = min(max(r, lo), hi)
    return q & ((1 << W) - 1)
