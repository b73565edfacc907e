"""The numpy model of float rows (sprintz_mi355x_float_rows, ChunkedCodec.float_rows): the only specification the mode has.

For element e of chunk c the column is d = e % ndims (chunk_len % ndims == 0; a short last chunk may end mid-row), and

    v   = x                         unsigned element, or sign-extended from 8 / 16 bits where `signed`
    f   = float32(v)                exact
    z   = fl32(fl32(f * scale[d]) + offset[d])      two roundings to nearest even, never one fma
    out = z                         F32
        = RNE(z) to binary16        F16   (overflow -> +-inf, subnormals kept)
        = RNE(z) to bfloat16        BF16  (subnormals kept), written (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the float32 bits u

The results are returned as BITS (uint32 for F32, uint16 for the two 16-bit formats): the tests compare bits, not values."""
import numpy as np

F32, F16, BF16 = 0, 1, 2
FORMATS = (F32, F16, BF16)
NAMES = {F32: "float32", F16: "float16", BF16: "bfloat16"}
OUT_BYTES = {F32: 4, F16: 2, BF16: 2}
BITS_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}

# (scale, offset): identity; the inverse of the uint16 range; a typical dequantisation; results that overflow float32 to inf; results that
# are float32 subnormals; a negative scale with a tiny offset; subnormal results with a subnormal offset; a scale with ties in bfloat16
PAIRS = [(1.0, 0.0), (1.0 / 65535, 0.0), (0.1, -3276.8), (3e38, 1.0), (2.0 ** -140, 0.0), (-7.3e-3, 1e-30), (2.0 ** -133, 2.0 ** -149),
         (1.0009765625, 0.5)]


def column_params(ndims):
    """column d takes pair d % 8 of PAIRS, so that a value converted with another column's parameters shows -> (scale, offset) float32 [ndims]"""
    s = np.array([PAIRS[d % len(PAIRS)][0] for d in range(ndims)], np.float32)
    o = np.array([PAIRS[d % len(PAIRS)][1] for d in range(ndims)], np.float32)
    return s, o


def values(x, signed):
    """the elements as float32, exactly"""
    x = np.asarray(x)
    assert x.dtype in (np.uint8, np.uint16)
    if signed:
        x = x.view(np.int8 if x.dtype == np.uint8 else np.int16)
    return x.astype(np.float32)


def affine(f, scale, offset):
    """fl32(fl32(f * scale) + offset): numpy rounds each float32 operation on its own"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m = (f * np.asarray(scale, np.float32)).astype(np.float32)
        return (m + np.asarray(offset, np.float32)).astype(np.float32)


def to_bits(z, fmt):
    z = np.ascontiguousarray(z, np.float32)
    if fmt == F32:
        return z.view(np.uint32).copy()
    if fmt == F16:
        with np.errstate(over="ignore", under="ignore"):
            return z.astype(np.float16).view(np.uint16)
    u = z.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def convert(x, scale, offset, signed, fmt):
    """elementwise: x and scale / offset broadcast against each other -> bits"""
    return to_bits(affine(values(x, signed), scale, offset), fmt)


def float_rows(x, chunk_len, ndims, scale=None, offset=None, signed=False, fmt=F32):
    """the batch x (its chunks back to back, the last one possibly short) -> bits of x.size elements.  Element e of chunk c is element
    c * chunk_len + e of x and of the result, in column e % ndims"""
    assert chunk_len % ndims == 0
    x = np.asarray(x).reshape(-1)
    scale = np.ones(ndims, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(ndims)
    offset = np.zeros(ndims, np.float32) if offset is None else np.asarray(offset, np.float32).reshape(ndims)
    d = (np.arange(x.size, dtype=np.int64) % chunk_len) % ndims
    return convert(x, scale[d], offset[d], signed, fmt)


def float_rows_brute(x, chunk_len, ndims, scale, offset, signed, fmt):
    """the same, one element at a time, chunk by chunk"""
    x = np.asarray(x).reshape(-1)
    out = np.zeros(x.size, BITS_DTYPE[fmt])
    W = 8 * x.dtype.itemsize
    for c in range(-(-x.size // chunk_len)):
        for e in range(min(chunk_len, x.size - c * chunk_len)):
            d = e % ndims
            v = int(x[c * chunk_len + e])
            if signed and v >= 1 << (W - 1):
                v -= 1 << W
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                z = np.float32(np.float32(np.float32(v) * np.float32(scale[d])) + np.float32(offset[d]))
            out[c * chunk_len + e] = to_bits(np.array([z], np.float32), fmt)[0]
    return out
