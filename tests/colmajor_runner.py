"""What the tests of the column-major kernels share (BASELINE config 5: encode_fast.h / encode_wide.h / decode_fast.h with CM = true, and the
generic pair): the three C entry points on sentinel-filled buffers with guard bands, the checkers -- the oracle's streams and return values on
the encode side, the input matrix and an untouched rest of the WHOLE buffer on the decode side, and the launches' kernel families against the
planner's answer for the call (tests/plan_probe.cpp) -- and the tables of the GPU tier's cases with the family each must run on, which the
CPU tier (tests/test_colmajor_cpu.py) replays through the planner without a device.  Nothing here imports torch or the library at import time."""
import ctypes as C
import os
import zlib
from contextlib import contextmanager
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import planner
from dispatch import check as check_dispatch, counts, moved
from harness import DTYPES
from streams import DENSE, options

PAD = 1024                                             # sentinel elements in front of and behind the matrix
BYTE = 0xA5
RETS_SENT = -77                                        # behind the last entry of rets, sizes and offsets
DENSE_PAD = 64                                         # sentinel bytes behind the container's capacity
CODEC_ID = {"delta": 0, "xff": 1}
BOTH = ("delta", "xff")


def sent(esz):
    """0xA5 repeated over an element"""
    return int.from_bytes(bytes([BYTE]) * esz, "little")


def chunks_of(nrows, R):
    return -(-nrows // R)


# ------------------------------------------------------------------ the planner's answers

@lru_cache(maxsize=None)
def encode_plan(codec, esz, D, R, nrows, cs, pair=1, no_fast=0, src_lo=0):
    shape = planner.plan_shape(codec, 8 * esz, D, R * D, chunks_of(nrows, R), pair=pair, no_fast=no_fast)
    shape["total_len"] = nrows * D
    return planner.ask("encode", col_stride=cs, src_lo=src_lo, **shape)


@lru_cache(maxsize=None)
def decode_plan(codec, esz, D, R, nchunks, cs, no_fast=0, cpg=1, out_lo=0):
    shape = planner.plan_shape(codec, 8 * esz, D, R * D, nchunks, no_fast=no_fast)
    return planner.ask("decode", col_stride=cs, out_lo=out_lo, chunks_per_group=cpg, **shape)


def min_fast_rows(esz, D, at_least=8):
    """the smallest multiple of 8 rows a chunk at which the planner sends a column-major decode to decode_fast.h"""
    R = at_least
    while decode_plan("xff", esz, D, R, 6, 1 << 20).get("family") != "dec_fast":
        R += 8
        assert R < 4096, (esz, D)
    return R


@contextmanager
def knobs(pair=1, no_fast=0, cpg=1):
    """SPRINTZ_OPT_ENC_PAIR, _NO_FAST and _CHUNKS_PER_GROUP for a call, restored afterwards"""
    from sprintz_amd import _lib
    with options(pair=pair, no_fast=no_fast):
        _lib.check(_lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, cpg))
        try:
            yield
        finally:
            _lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(os.environ.get("SPRINTZ_MI355X_CHUNKS_PER_GROUP", 1)))


# ------------------------------------------------------------------ the matrix and the oracle's side

def matrix(rows, cs, shift=0, tight=False):
    """-> (flat host buffer, offset of element (0, 0)): [D, cs] with rows.T in its first nrows columns and the sentinel everywhere else -- PAD +
    shift elements in front and PAD behind; tight: nothing in front, and behind only the READ_SLACK bytes the header asks of a source"""
    nrows, D = rows.shape
    esz = rows.dtype.itemsize
    front, back = (0, 16 // esz) if tight else (PAD + shift, PAD)
    m = np.full(front + D * cs + back, sent(esz), DTYPES[esz])
    m[front:front + D * cs].reshape(D, cs)[:, :nrows] = rows.T
    return m, front


_EXPECTED = {}


def expected(oracle, codec, rows, R):
    """-> (the oracle's stream of every chunk of the row-major flattening, the reference's return value of every chunk)"""
    rows = np.ascontiguousarray(rows)
    key = (codec, R, rows.shape, rows.dtype.itemsize, zlib.crc32(rows.tobytes()))
    if key not in _EXPECTED:
        D = rows.shape[1]
        flat = rows.reshape(-1)
        streams = oracle.compress_chunks(codec, flat, R * D, D) if flat.size else []
        rets = [oracle.compress(codec, flat[c * R * D:(c + 1) * R * D], D)[1] for c in range(len(streams))]
        _EXPECTED[key] = (streams, rets)
    return _EXPECTED[key]


def to_device(a):
    import torch
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16}[a.dtype.itemsize]).copy()).cuda()


# ------------------------------------------------------------------ encode

def encode(sz, rows, codec, R, cs=None, shift=0, tight=False, dense=True, pair=1, no_fast=0, stream=None, bufs=None):
    """compress_batch_colmajor[_dense] on rows [nrows, D] laid out as matrix(...): slots, sizes, rets (and offsets) carry one sentinel entry
    behind their last, the container DENSE_PAD sentinel bytes behind its capacity.  bufs: an earlier call's buffers, used again dirty.
    -> the results on the host, the families that moved, and (dense) the container as a CompressedBatch"""
    import torch
    _lib = sz._lib
    rows = np.ascontiguousarray(rows)
    nrows, D = rows.shape
    esz = rows.dtype.itemsize
    cs = nrows if cs is None else cs
    n = chunks_of(nrows, R)
    ss = int(_lib.compress_bound(esz, R * D, D))
    if bufs is None:
        m, front = matrix(rows, cs, shift, tight)
        bufs = dict(src=to_device(m), host=m, front=front,
                    slots=torch.full(((n + 1) * ss,), BYTE, dtype=torch.uint8, device="cuda"),
                    sizes=torch.full((n + 1,), RETS_SENT, dtype=torch.int32, device="cuda"),
                    rets=torch.full((n + 1,), RETS_SENT, dtype=torch.int64, device="cuda"))
        if dense:
            bufs.update(dense=torch.full((n * ss + _lib.READ_SLACK + DENSE_PAD,), BYTE, dtype=torch.uint8, device="cuda"),
                        offsets=torch.full((n + 2,), RETS_SENT, dtype=torch.int64, device="cuda"),
                        tmp=torch.empty((int(_lib.compress_dense_tmp_bytes(max(n, 1))),), dtype=torch.uint8, device="cuda"))
    src = bufs["src"].data_ptr() + bufs["front"] * esz
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    with knobs(pair=pair, no_fast=no_fast), torch.cuda.stream(st):
        before = counts()
        common = (CODEC_ID[codec], esz, src, nrows, cs, R, D, bufs["slots"].data_ptr(), ss, bufs["sizes"].data_ptr(), bufs["rets"].data_ptr())
        if dense:
            _lib.check(_lib.compress_batch_colmajor_dense(*common, bufs["dense"].data_ptr(), bufs["offsets"].data_ptr(), bufs["tmp"].data_ptr(),
                                                          C.c_void_p(st.cuda_stream)))
        else:
            _lib.check(_lib.compress_batch_colmajor(*common, C.c_void_p(st.cuda_stream)))
        ran = moved(before, counts())
    torch.cuda.synchronize()
    res = SimpleNamespace(ran=ran, n=n, ss=ss, esz=esz, D=D, R=R, nrows=nrows, cs=cs, dense=dense, bufs=bufs, src_lo=src & 15,
                          plan=encode_plan(codec, esz, D, R, nrows, cs, pair, no_fast, src & 15) if n else None,
                          slots=bufs["slots"].cpu().numpy(), sizes=bufs["sizes"].cpu().numpy(), rets=bufs["rets"].cpu().numpy(), batch=None)
    res.family = res.plan["family"] if n else None
    if dense:
        res.container, res.offsets = bufs["dense"].cpu().numpy(), bufs["offsets"].cpu().numpy()
        if n and 0 <= res.offsets[n] <= n * ss:
            total = int(res.offsets[n])
            res.batch = sz.CompressedBatch(bufs["dense"][:total + _lib.READ_SLACK].clone(), bufs["offsets"][:n + 1].clone(), bufs["sizes"][:n].clone(),
                                           n, nrows * D, R * D, D)
    return res


def check_encode(res, oracle, codec, rows, tag):
    """every chunk's size and bytes are the oracle's -- in its slot and, dense, in the container, whose offsets are the sizes' 16-byte aligned
    prefix sums --, rets the reference's return values; the entries behind the last, the slot behind the last, the container behind its capacity
    and the source are untouched; the encoder's family is the planner's and nothing else but the container's passes launched"""
    n, ss = res.n, res.ss
    want, rets = expected(oracle, codec, rows, res.R)
    assert len(want) == n, (tag, n, len(want))
    at = 0
    for c, w in enumerate(want):
        assert res.sizes[c] == w.size, (tag, "chunk", c, "size", int(res.sizes[c]), "the oracle's", w.size)
        assert np.array_equal(res.slots[c * ss:c * ss + w.size], w), (tag, "chunk", c, "differs from the oracle's stream")
        assert res.rets[c] == rets[c], (tag, "chunk", c, "rets", int(res.rets[c]), "the reference's", rets[c])
        if res.dense:
            assert res.offsets[c] == at, (tag, "chunk", c, "offset", int(res.offsets[c]), at)
            assert np.array_equal(res.container[at:at + w.size], w), (tag, "chunk", c, "differs from the oracle's stream in the container")
            at = (at + w.size + 15) & ~15
    assert res.sizes[n] == RETS_SENT and res.rets[n] == RETS_SENT, (tag, "written behind the last entry", res.sizes[n:], res.rets[n:])
    assert (res.slots[n * ss:] == BYTE).all(), (tag, "written behind the last slot")
    if res.dense:
        if n:
            assert res.offsets[n] == at, (tag, "the container's end", int(res.offsets[n]), at)
        assert res.offsets[n + 1] == RETS_SENT, (tag, "written behind the last offset")
        assert (res.container[n * ss + 16:] == BYTE).all(), (tag, "written behind the container's capacity")
    assert np.array_equal(res.bufs["src"].cpu().numpy().view(res.bufs["host"].dtype), res.bufs["host"]), (tag, "the source changed")
    if n == 0:
        check_dispatch(res.ran, only=[], what=str(tag))
    else:
        check_dispatch(res.ran, {res.family: 1}, only=[res.family, *DENSE] if res.dense else [res.family], what=str(tag))


# ------------------------------------------------------------------ decode

def decode(sz, batch, codec, esz, D, R, cs, shift=0, tight=False, no_fast=0, cpg=1, stream=None, bufs=None, nchunks=None):
    """decompress_batch_colmajor into a sentinel-filled [D, cs] with PAD + shift elements in front and PAD behind (tight: none), rets one
    sentinel entry behind.  -> the whole buffer and rets on the host, the families that moved"""
    import torch
    _lib = sz._lib
    n = batch.nchunks if nchunks is None else nchunks
    front, back = (0, 0) if tight else (PAD + shift, PAD)
    if bufs is None:
        bufs = dict(out=torch.full(((front + D * cs + back) * esz,), BYTE, dtype=torch.uint8, device="cuda"),
                    rets=torch.full((n + 1,), RETS_SENT, dtype=torch.int64, device="cuda"))
    dst = bufs["out"].data_ptr() + front * esz
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    with knobs(no_fast=no_fast, cpg=cpg), torch.cuda.stream(st):
        before = counts()
        _lib.check(_lib.decompress_batch_colmajor(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, R, D, cs, dst,
                                                  bufs["rets"].data_ptr(), C.c_void_p(st.cuda_stream)))
        ran = moved(before, counts())
    torch.cuda.synchronize()
    res = SimpleNamespace(ran=ran, n=n, esz=esz, D=D, R=R, cs=cs, front=front, bufs=bufs, out_lo=dst & 15,
                          plan=decode_plan(codec, esz, D, R, n, cs, no_fast, cpg, dst & 15) if n else None,
                          out=bufs["out"].cpu().numpy().view(DTYPES[esz]), rets=bufs["rets"].cpu().numpy())
    res.family = res.plan["family"] if n else None
    return res


def check_decode(res, rows, tag, bad=()):
    """the WHOLE buffer is rows.T inside the sentinel -- the rows past nrows of every column, the stride's padding and both guard bands are
    untouched --, with rows [c R, (c + 1) R) of every column left out for a damaged chunk c in `bad`, whose own output is unspecified; rets are
    the chunks' element counts, negative in `bad`, the sentinel behind; the decoder's family is the planner's and nothing else launched"""
    nrows, D = rows.shape
    cs, R, n = res.cs, res.R, res.n
    want = np.full(res.out.size, sent(res.esz), res.out.dtype)
    want[res.front:res.front + D * cs].reshape(D, cs)[:, :nrows] = rows.T
    keep = np.ones(res.out.size, bool)
    for c in bad:
        keep[res.front:res.front + D * cs].reshape(D, cs)[:, c * R:(c + 1) * R] = False
    diff = np.flatnonzero((res.out != want) & keep)
    if diff.size:
        e = int(diff[0]) - res.front
        where = "the front guard" if e < 0 else "the back guard" if e >= D * cs else \
            f"column {e // cs} row {e % cs} (chunk {e % cs // R}, nrows {nrows}, col_stride {cs})"
        raise AssertionError((tag, int(diff.size), "elements differ; first in", where, "got", int(res.out[diff[0]]), "want", int(want[diff[0]])))
    lens = [min(R, nrows - c * R) * D for c in range(n)]
    assert all(res.rets[c] == lens[c] for c in range(n) if c not in bad) and all(res.rets[c] < 0 for c in bad) and res.rets[n] == RETS_SENT, \
        (tag, "rets", res.rets.tolist(), "counts", lens, "damaged", list(bad))
    if n == 0:
        check_dispatch(res.ran, only=[], what=str(tag))
    else:
        check_dispatch(res.ran, {res.family: 1}, only=[res.family], what=str(tag))


def wrong_ndims(batch, c, D):
    """a copy of the container with another ndims in bytes 6 .. 7 of chunk c's stream header"""
    import torch
    data = batch.data.clone()
    off = int(batch.offsets[c].item())
    wrong = D ^ 5
    data[off + 6:off + 8] = torch.tensor([wrong & 0xFF, wrong >> 8], dtype=torch.uint8, device="cuda")
    return type(batch)(data, batch.offsets, batch.sizes, batch.nchunks, batch.total_len, batch.chunk_len, batch.ndims)


# ------------------------------------------------------------------ data

def walk(seed, nrows, D, esz, R, flat=True):
    """[nrows, D]: a +-6 random walk a column; flat: held constant over a span that crosses the seam between chunks 1 and 2"""
    rng = np.random.default_rng(seed)
    top = 1 << (8 * esz)
    steps = rng.integers(-6, 7, (nrows, D))
    steps[steps == 0] = 1                               # (no block is all zero by chance: a chunk's stream groups are then its blocks' alone)
    if flat and nrows > 2 * R + 24:
        steps[2 * R - 40:2 * R + 24] = 0
    return ((np.cumsum(steps, axis=0) + rng.integers(0, top, (1, D))) % top).astype(DTYPES[esz])


# ------------------------------------------------------------------ the GPU tier's tables (tests/test_gpu_colmajor*.py), replayed by the CPU tier

# tests/test_gpu_colmajor.py: name, codec, esz, ndims, rows_per_chunk, nrows, col_stride (0 = nrows), then the families of the encoder with two
# columns a lane asked for (SPRINTZ_OPT_ENC_PAIR 1), with one (0), and of the decoder
CM_CONFIGS = [
    ("cfg5 u16 D=32 xff 160-row chunks (fast kernels)", "xff", 2, 32, 160, 160 * 41 + 57, 160 * 42, "enc_pair", "enc_fast", "dec_fast"),
    ("u16 D=8 xff 640-row chunks", "xff", 2, 8, 640, 640 * 20, 0, "enc_pair", "enc_fast", "dec_fast"),
    ("u16 D=8 delta", "delta", 2, 8, 640, 640 * 7 + 8, 640 * 8, "enc_pair", "enc_fast", "dec_fast"),
    ("u8 D=16 xff", "xff", 1, 16, 256, 256 * 9 + 100, 256 * 10 + 8, "enc_pair", "enc_fast", "dec_fast"),
    ("u8 D=64 delta", "delta", 1, 64, 128, 128 * 12, 0, "enc_pair", "enc_fast", "dec_fast"),
    ("u16 D=5 (generic kernels: odd column count)", "xff", 2, 5, 200, 200 * 6 + 33, 0, "enc_generic", "enc_generic", "dec_fast"),   # (the encoders: nrows is the stride, and odd; the test's destination has a stride of whole blocks)
    ("u16 D=8, unaligned stride (generic kernels)", "xff", 2, 8, 100, 100 * 9 + 3, 903, "enc_generic", "enc_generic", "dec_generic"),
    ("u8 D=2 low-dim", "delta", 1, 2, 512, 512 * 5 + 1, 0, "enc_generic", "enc_generic", "dec_generic"),
    ("u16 D=100 (2 columns per lane)", "xff", 2, 100, 64, 64 * 7 + 5, 64 * 8, "enc_generic", "enc_generic", "dec_fast"),
    ("u16 D=6 (fast kernels, group not full)", "xff", 2, 6, 160, 160 * 9 + 48, 160 * 10, "enc_pair", "enc_fast", "dec_fast"),
    ("u8 D=12 (fast kernels, group not full)", "delta", 1, 12, 256, 256 * 5 + 64, 256 * 6, "enc_pair", "enc_fast", "dec_fast"),
    ("u16 D=48 delta (fast kernels, group not full)", "delta", 2, 48, 104, 104 * 11 + 16, 104 * 12, "enc_pair", "enc_fast", "dec_fast"),
]

# (pair, no_fast, family) of an encode leg, (no_fast, chunks_per_group, family) of a decode leg
ENC_FAST_LEGS = [(1, 0, "enc_pair"), (0, 0, "enc_fast"), (1, 1, "enc_generic")]
ENC_GENERIC_LEGS = [(1, 0, "enc_generic"), (0, 0, "enc_generic"), (1, 1, "enc_generic")]       # (no column-major kernel above 64 columns, nor for the low-dim shapes)
DEC_FAST_LEGS = [(0, 1, "dec_fast"), (0, 3, "dec_fast"), (1, 1, "dec_generic")]
DEC_GENERIC_LEGS = [(0, 1, "dec_generic"), (1, 1, "dec_generic")]

# the run drive's shapes: (w, D) -> what the shape is there for, the encode legs, the decode legs
RLE_SHAPES = {
    (16, 8): ("one column a lane, exact", ENC_FAST_LEGS, DEC_FAST_LEGS),
    (16, 6): ("one column a lane, lanes without a column", ENC_FAST_LEGS, DEC_FAST_LEGS),
    (8, 12): ("one column a lane, lanes without a column", ENC_FAST_LEGS, DEC_FAST_LEGS),
    (8, 32): ("one column a lane, 8-byte pieces", ENC_FAST_LEGS, DEC_FAST_LEGS),
    (16, 100): ("two columns a lane", ENC_GENERIC_LEGS, DEC_FAST_LEGS),
    (8, 100): ("two columns a lane", ENC_GENERIC_LEGS, DEC_FAST_LEGS),
}
RLE_NCHUNKS, RLE_NB = 16, 256                          # the run drive's batch: 16 rotations of 256 blocks

# the FIRE drive's shapes (drive_tables.FIRE_SHAPES: 8 bits x 8, every counter wraps; 16 bits x 1, the low-dim layout -- generic on both sides)
FIRE_LEGS = {
    (8, 8): (ENC_FAST_LEGS, DEC_FAST_LEGS),
    (16, 1): (ENC_GENERIC_LEGS, DEC_GENERIC_LEGS),
}

# every lane mapping of decode_fast.h: D -> (lanes a chunk, columns a lane); MAP_ROWS rows a chunk at both widths (six groups and a block;
# tests/test_colmajor_cpu.py: the planner takes it at every D), 7 chunks, the last one ragged
MAPPINGS = {5: (8, 1), 8: (8, 1), 12: (16, 1), 16: (16, 1), 24: (32, 1), 32: (32, 1), 48: (64, 1), 64: (64, 1),
            65: (64, 2), 100: (64, 2), 128: (64, 2), 129: (64, 4), 200: (64, 4), 256: (64, 4)}
MAP_ROWS, MAP_NCHUNKS, MAP_LAST = 104, 7, 29
MAP_ENCODE_MAX = 64                                    # the column-major encoders' widest shape

# step parity: (w, D) -> rows a chunk with (stream groups, rows behind them) of a full chunk -- an odd and an even number of groups, each with
# and without eight more rows: the smallest multiples of 8 the planner takes with those residues (tests/test_colmajor_cpu.py pins the first as
# the planner's boundary and counts the groups in the oracle's streams)
PARITY_ROWS = {
    (16, 8): {56: (3, 8), 64: (4, 0), 72: (4, 8), 80: (5, 0)},
    (8, 16): {64: (4, 0), 72: (4, 8), 80: (5, 0), 88: (5, 8)},
}
PARITY_NCHUNKS = 6                                     # at three chunks a lane group the short chunk ends the second group


def parity_data(w, D, R, last):
    """five chunks of R rows and one of `last`, no block all zero: a chunk's groups are its blocks' alone"""
    return walk(R * 100 + last, (PARITY_NCHUNKS - 1) * R + last, D, w // 8, R, flat=False)


def parity_lasts(R):
    """rows of the last chunk -> (stream groups, rows behind them): nothing but a tail, one block, one group, a group and a tail"""
    return {1: (0, 1), 7: (0, 7), 8: (0, 8), 15: (0, 15), 16: (1, 0), 17: (1, 1), R - 1: ((R - 1) // 16, (R - 1) % 16)}


# damage: (w, D, no_fast) -> family; DAMAGE_ROWS rows a chunk, 8 chunks, chunk 4 damaged -- at three chunks a group the middle one of the second
DAMAGE_SHAPES = {(16, 8, 0): "dec_fast", (8, 32, 0): "dec_fast", (16, 100, 0): "dec_fast", (16, 8, 1): "dec_generic"}
DAMAGE_ROWS, DAMAGE_NCHUNKS, DAMAGE_BAD = 72, 8, 4

# reach.  Decode, uint16 x 8, five chunks of the smallest R the planner takes: the largest multiple of 8 with D cs esz < 0xf0000000, and the next
REACH_DEC = dict(esz=2, D=8, R=56, nchunks=5, cs_fast=0xf0000000 // 16 - 8, cs_generic=0xf0000000 // 16)
# encode, uint8 x 5, three chunks: a stride that does not fit 32 bits
REACH_ENC = dict(esz=1, D=5, R=64, nchunks=3, cs=(1 << 32) + 64)
